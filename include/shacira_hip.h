/*
 * shacira_hip.h -- C-ABI of libshacira_hip.so, the MI355X (gfx950) implementation of SHACIRA's hash-grid
 * interpolation and latent quantisation / entropy path.
 *
 * This is the drop-in boundary: exactly the operators the reference binds through pybind11 in
 * wisp/csrc/bindings.cpp:24-28 (declared in wisp/csrc/ops/hashgrid_interpolate.h:18-50), restated with plain
 * pointers and sizes (no ATen types), plus the per-entry latent decode / entropy-bit operators that the
 * reference evaluates as chains of ATen elementwise kernels
 * (wisp/models/latent_decoders/basic_latent_decoder.py:182-198, wisp/models/grids/latent_grid.py:122-136,
 * wisp/models/prob_models/bit_estimator.py:27-65).
 *
 * Conventions (all entry points):
 *   - every buffer is CALLER-OWNED device memory (hipMalloc / the PyTorch caching allocator) unless the name
 *     ends in _host; the library never allocates or frees device memory and never synchronises the host (the backward
 *     of large batches with LDS-resident levels (3-D: n * L * F >= 7 * 2^21, 2-D: >= 2^23) creates, once per host thread and
 *     device, one non-blocking side stream and three events that it forks from / joins back into `stream`: stream semantics are unchanged, HIP-graph capture works
 *     after one eager call). Those objects belong to the CURRENT device (hipGetDevice): like every HIP launch, a call
 *     must be made with the device of `stream` and of its buffers current;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream) and the call
 *     returns immediately; calls are reentrant and thread-safe (the backward runs on autograd worker threads);
 *   - return value: 0 on success, a negative SHACIRA_E* code for invalid arguments (nothing enqueued), or a
 *     positive hipError_t if the launch failed. shacira_strerror() describes either;
 *   - tensors are dense row-major.
 */
#ifndef SHACIRA_HIP_H
#define SHACIRA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHACIRA_ABI_VERSION 11

#if defined(__GNUC__)
#define SHACIRA_API __attribute__((visibility("default")))
#else
#define SHACIRA_API
#endif

/* table / feature scalar types (AT_DISPATCH_FLOATING_TYPES_AND_HALF in hashgrid_interpolate_cuda.cu:125) */
#define SHACIRA_F32 0
#define SHACIRA_F16 1
/* double tables (the third type of the reference's dispatch macro, .cu:125,290). Forward: every table value narrowed to
 * float, fp32 interpolation, result widened (.cu:96-107) -- the reference-shaped kernel only. Backward: (float)(grad * weight)
 * accumulated with atomicAdd(double). NOTE the reference's own double backward is broken: .cu:212-221 adds a float through
 * `(float*)(grad_codebook + ...)`, i.e. into the LOW WORD of each double; this library computes the intended gradient. */
#define SHACIRA_F64 2

#define SHACIRA_MAX_LODS 32

#define SHACIRA_EINVAL   (-1) /* bad dim / sizes / bitwidth / null pointer              */
#define SHACIRA_EDTYPE   (-2) /* unsupported scalar type                                */
#define SHACIRA_EODD     (-3) /* feature_dim is odd (wisp/ops/grid.py:75-76 raises too) */
#define SHACIRA_EWORKSPACE (-4) /* workspace too small for the requested algorithm      */

SHACIRA_API int shacira_abi_version(void);
SHACIRA_API const char *shacira_strerror(int code);

/*
 * Forward: replaces hashgrid_interpolate_cuda / hashgrid_interpolate2d_cuda
 * (wisp/csrc/ops/hashgrid_interpolate.cpp:44-66 and :130-152; kernels hashgrid_interpolate_cuda.cu:47-109,
 * hashgrid_interpolate2d_cuda.cu:44-99). All levels are evaluated by one launch.
 *
 *   dim                2 or 3 (coords are [num_coords, dim] fp32 in [-1, 1])
 *   codebook           [table_rows, feature_dim] of `dtype`; levels concatenated, level l starts at row
 *                      codebook_first_idx[l]
 *   codebook_first_idx DEVICE int32 [num_lods] (the module's `codebook_lod_first_idx` buffer)
 *   resolutions_host   HOST int32 [num_lods] (the Python list the reference converts to std::vector<int32_t>)
 *   feats              out, [num_coords, num_lods*feature_dim] of `dtype` (level-major, feature-minor)
 *   table_rows         total rows; used only to keep the reference's out-of-table corner (coord == +1 on a
 *                      dense level with res >= 258, weight 0) memory-safe
 *   workspace          scratch of at least shacira_hashgrid_forward_workspace_bytes(...) bytes (level-major staging
 *                      of the features, and the sample sort of large batches; may be NULL when that returns 0)
 */
SHACIRA_API size_t shacira_hashgrid_forward_workspace_bytes(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                int codebook_bitwidth, const int32_t *resolutions_host,
                                                int64_t table_rows, int dtype);

SHACIRA_API int shacira_hashgrid_forward(int dim, int64_t num_coords, int num_lods, int feature_dim, int codebook_bitwidth,
                             const int32_t *resolutions_host, const int32_t *codebook_first_idx,
                             int64_t table_rows, const float *coords, const void *codebook, int dtype,
                             void *feats, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Test hook (not used by any caller of the operators): the integers and weights behind one lookup, so that "hash
 * indices bit-exact" can be checked directly instead of through the features. For every (sample, level):
 *   corner_rows    int32 [num_coords, num_lods, 2^dim]  level-local row of corner k, i.e. hash_index / hash_index2d of
 *                  the reference (hashgrid_interpolate_cuda.cu:17-39, hashgrid_interpolate2d_cuda.cu:17-36) applied to
 *                  the corner positions of .cu:86-94 (k: bit2 -> x, bit1 -> y, bit0 -> z; 2-D: bit1 -> x, bit0 -> y)
 *   corner_weights fp32  [num_coords, num_lods, 2^dim]  the weight products of .cu:77-84 / 2d.cu:72-75
 * computed by the same device function every forward / backward kernel of this library uses. Either output may be NULL.
 */
SHACIRA_API int shacira_hashgrid_debug_corners(int dim, int64_t num_coords, int num_lods, int codebook_bitwidth,
                                   const int32_t *resolutions_host, const float *coords, int32_t *corner_rows,
                                   float *corner_weights, void *stream);

/*
 * Backward: replaces hashgrid_interpolate_backward_cuda / hashgrid_interpolate2d_backward_cuda
 * (hashgrid_interpolate.cpp:68-100 and :154-186; kernels .cu:143-221, 2d.cu:133-208).
 *
 *   grad_output    [num_coords, num_lods*feature_dim] of `dtype`
 *   grad_codebook  out, [table_rows, feature_dim] of `dtype`; the call overwrites it completely
 *                  (the reference's at::zeros_like + atomicAdd), no pre-zeroing needed
 *   workspace      scratch of at least shacira_hashgrid_backward_workspace_bytes(...) bytes (may be NULL if 0)
 *
 * The gradient with respect to the coordinates is a separate call: shacira_hashgrid_coords_backward below.
 */
SHACIRA_API size_t shacira_hashgrid_backward_workspace_bytes(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                 int codebook_bitwidth, const int32_t *resolutions_host,
                                                 int64_t table_rows, int dtype);

SHACIRA_API int shacira_hashgrid_backward(int dim, int64_t num_coords, int num_lods, int feature_dim, int codebook_bitwidth,
                              const int32_t *resolutions_host, const int32_t *codebook_first_idx,
                              int64_t table_rows, const float *coords, const void *grad_output, int dtype,
                              void *grad_codebook, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Same, restricted to levels [level_begin, level_end): writes (completely) only the rows of those levels,
 * [codebook_first_idx[level_begin], codebook_first_idx[level_end]) (to table_rows for level_end == num_lods), and leaves
 * the rest of grad_codebook untouched. Lets a data-parallel caller start the all-reduce of the finished rows while the
 * remaining levels are still being computed. fp32 tables, and fp16 tables without the two flags below (a half table converts
 * only the call's own rows of its fp32 accumulation image); double tables take whole calls. Same workspace size as the full call.
 *   flags: SHACIRA_BWD_STAGE_ALL_LEVELS  stage (transpose) the gradients of ALL levels into the workspace, not only
 *                                        this call's, so that later calls on the SAME workspace can skip that pass;
 *          SHACIRA_BWD_REUSE_STAGED      the workspace already holds them (set by an earlier call with the flag above,
 *                                        same arguments, same workspace, same stream order).
 */
#define SHACIRA_BWD_STAGE_ALL_LEVELS 1
#define SHACIRA_BWD_REUSE_STAGED 2
SHACIRA_API int shacira_hashgrid_backward_levels(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                     int codebook_bitwidth, const int32_t *resolutions_host,
                                     const int32_t *codebook_first_idx, int64_t table_rows, const float *coords,
                                     const void *grad_output, int dtype, void *grad_codebook, int level_begin,
                                     int level_end, int flags, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The PLAN of a coordinate batch (round 6, ABI 10): forward and backward of one training step see the same coordinates
 * (the reference saves `coords` for the backward, wisp/ops/grid.py:86,106) -- what the forward of a large batch computes
 * first, the batch counting-sorted by spatial block (16-byte records {x, y, z, sample index} + block offsets), is exactly
 * what lets the backward accumulate its coarse levels block by block on chip instead of through the item stream. The two
 * calls below are shacira_hashgrid_forward / shacira_hashgrid_backward with one more CALLER-OWNED buffer: the forward
 * writes the batch's plan into it, the backward of the same (dim, num_coords, coords) reads it. Results are those of the
 * plain calls (forward: bit-identical; backward: the same products, summed in a different order).
 *
 *   shacira_hashgrid_plan_bytes      size of the plan buffer for this shape; 0 = the forward of this shape sorts nothing
 *                                    (small batches, cache-resident tables): pass plan = NULL, the calls are the plain ones
 *   plan                             device buffer of at least that size (256-byte aligned), or NULL. The forward overwrites
 *                                    it; the backward only reads it. A plan is a function of (dim, num_coords, coords): a
 *                                    caller that trains on a FIXED batch (the reference's image trainer revisits the same
 *                                    pixel lattice every step, wisp/trainers/image_trainer.py:234-266) may keep it across
 *                                    steps and pass plan_flags = SHACIRA_PLAN_READY to the forward, which then skips its sort
 *   plan_bytes                       size of the buffer; SHACIRA_EWORKSPACE when it is non-NULL and too small
 *   workspace (forward)              shacira_hashgrid_forward_workspace_bytes covers a call without a plan buffer, which keeps
 *                                    its plan inside the workspace; a forward that brings its plan buffer (plan != NULL, a shape
 *                                    that sorts) accepts a workspace shorter by shacira_hashgrid_plan_bytes
 *   shacira_hashgrid_backward_planned_workspace_bytes (ABI 11)
 *                                    scratch the planned backward of this shape needs: the levels its brick pass takes write no
 *                                    items and the others 12-byte units, S1 at 2^20 samples: 0.70 GB against the 1.10 GB of
 *                                    shacira_hashgrid_backward_workspace_bytes (which such a call accepts, too). Holds for a
 *                                    16-byte aligned grad_output; a planned call on an unaligned one runs the plain passes
 *                                    and asks for the plain size (SHACIRA_EWORKSPACE below it). Equal to the plain size for
 *                                    shapes without a plan or outside the brick pass's rule.
 */
#define SHACIRA_PLAN_READY 1
SHACIRA_API size_t shacira_hashgrid_plan_bytes(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                               int codebook_bitwidth, const int32_t *resolutions_host, int64_t table_rows,
                                               int dtype);
SHACIRA_API size_t shacira_hashgrid_backward_planned_workspace_bytes(int dim, int64_t num_coords, int num_lods,
                                                                     int feature_dim, int codebook_bitwidth,
                                                                     const int32_t *resolutions_host, int64_t table_rows,
                                                                     int dtype);
SHACIRA_API int shacira_hashgrid_forward_planned(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                 int codebook_bitwidth, const int32_t *resolutions_host,
                                                 const int32_t *codebook_first_idx, int64_t table_rows, const float *coords,
                                                 const void *codebook, int dtype, void *feats, void *plan, size_t plan_bytes,
                                                 int plan_flags, void *workspace, size_t workspace_bytes, void *stream);
SHACIRA_API int shacira_hashgrid_backward_planned(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                  int codebook_bitwidth, const int32_t *resolutions_host,
                                                  const int32_t *codebook_first_idx, int64_t table_rows, const float *coords,
                                                  const void *grad_output, int dtype, void *grad_codebook, const void *plan,
                                                  size_t plan_bytes, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Coordinate backward (ABI 11, additive): the gradient of the features with respect to the input coordinates. The reference's
 * `require_grad_coords` branch (hashgrid_interpolate_cuda.cu:223-269) is dead code there (its result is never returned,
 * hashgrid_interpolate.cpp:84-96) and is not what is computed here. For sample n, level l, axis a, with the forward's own
 * transform u = (float)(res_l * ((double)c_a * 0.5 + 0.5)), x = clamp(u, 0, hi_l), frac = x - floor(x), the corner values
 * t[k, f] of compute_corners' level-local rows (the forward's out-of-table masking: such a corner reads as 0 and its row is
 * never read outside the table) and g = grad_output[n, l*F + f]:
 *
 *   grad_coords[n, a] = sum_l s_l,a * sum_f g[n,l,f] * sum_{corner pairs (k0, k1) that differ only in axis a} W_a(k0) * (t[k1,f] - t[k0,f])
 *   s_l,a  = 0.5 * res_l where 0 <= u <= hi_l (both ends inclusive: torch.clamp's autograd convention), 0 where the clamp
 *            acts and for NaN coordinates (the forward maps those to hi_l)
 *   W_a(k) = product of the other axes' weights (frac or 1 - frac, fp32, as in the forward's weights)
 *
 * At a cell boundary the derivative is the one-sided value of the cell floor() picks. fp32 arithmetic: fp16 tables and
 * gradients are widened, fp64 tables and gradients read as fp32 (the forward's Scalar<double>). ONE expression tree, explicit
 * fmaf (the library is built with -ffp-contract=off), corner k: bit dim-1-a -> axis a:
 *   D_f[a] = d(k0_0) * W(k0_0), then fmaf(d(k0), W(k0), D) over the pairs of axis a, k0 ascending, d(k0) = t[k1,f] - t[k0,f],
 *            W a left-to-right product of the other axes' weights in axis order
 *   S_l[a] = g_0 * D_0[a], then fmaf(g_f, D_f[a], S) for f ascending
 *   grad[a] = 0, then fmaf(s_l,a, S_l[a], grad[a]) for l ascending
 * Every kernel variant evaluates exactly this tree: the result for a sample depends on that sample only, so variants, sample
 * order and planned or plain calls agree bit for bit.
 *
 *   codebook        [table_rows, feature_dim] of `dtype` (the table the forward read)
 *   grad_output     [num_coords, num_lods*feature_dim] of `dtype`
 *   grad_coords     out, fp32 [num_coords, dim]; overwritten, not accumulated
 *   plan            NULL, or the buffer the planned forward of the same coordinates filled (the contract of
 *                   shacira_hashgrid_backward_planned; ignored for shapes whose forward sorts nothing; SHACIRA_EWORKSPACE when
 *                   plan_bytes is below shacira_hashgrid_plan_bytes). Lets large 3-D batches walk the samples in sorted order.
 *   workspace       scratch of shacira_hashgrid_coords_backward_workspace_bytes(...) bytes (0 today: may be NULL)
 * Validation happens before any HIP call, with the codes of shacira_hashgrid_forward; num_coords == 0 returns 0. No host
 * synchronisation and no allocation: safe to capture into a graph.
 */
SHACIRA_API size_t shacira_hashgrid_coords_backward_workspace_bytes(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                                    int codebook_bitwidth, const int32_t *resolutions_host,
                                                                    int64_t table_rows, int dtype);
SHACIRA_API int shacira_hashgrid_coords_backward(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                 int codebook_bitwidth, const int32_t *resolutions_host,
                                                 const int32_t *codebook_first_idx, int64_t table_rows, const float *coords,
                                                 const void *codebook, const void *grad_output, int dtype, float *grad_coords,
                                                 const void *plan, size_t plan_bytes, void *workspace,
                                                 size_t workspace_bytes, void *stream);

/*
 * Backward of the coordinate backward (ABI 11, additive): what a loss on the coordinate gradient (eikonal, normal
 * consistency, gradient matching) needs. The node differentiated is shacira_hashgrid_coords_backward above,
 *   gc[n,a] = sum_l s_l,a * sum_f g[n,l,f] * sum_k sigma_a(k) W_a(k) t[k,f]
 * in that comment's symbols, with sigma_a(k) = +1 if corner k's bit for axis a is set and -1 otherwise (the pair sum written
 * over single corners), W_a(k) = prod_{c != a} w_c(k) and W_ab(k) = prod_{c != a,b} w_c(k) (1 in 2-D), w_c(k) = frac if corner
 * k's bit for axis c is set, 1 - frac otherwise. Given v = dL/dgc (grad_grad_coords, fp32 [num_coords, dim]):
 *
 *   (1) grad_grad_output[n,l,f] = sum_a v_a s_l,a sum_k sigma_a(k) W_a(k) t[k,f]
 *       the directional derivative of the features along v: a gather (coords, v, the table; not g)
 *   (2) grad_codebook[first_l + row_k, f] += g[n,l,f] * sum_a v_a s_l,a sigma_a(k) W_a(k)
 *       the addresses of shacira_hashgrid_backward with the corner weight replaced by its directional derivative: a
 *       scatter-add (coords, v, g; not the table's values). Overwritten: the call zeroes it first, out-of-table corners are
 *       never touched
 *   (3) grad_coords[n,b] = sum_l sum_{a != b} v_a s_l,a s_l,b sum_f g[n,l,f] sum_k sigma_a(k) sigma_b(k) W_ab(k) t[k,f]
 *       the mixed second derivatives: a gather, fp32 [num_coords, dim], overwritten. The pure second derivatives are zero
 *       inside a cell, and the derivative of the slope s (zero almost everywhere) is taken as zero
 *
 * fp32 arithmetic on the forward's fp64 coordinate transform, explicit fmaf (-ffp-contract=off). (1) and (3) are ONE
 * expression tree each, evaluated by every kernel variant, so a sample's result depends on that sample alone and calls agree
 * bit for bit across runs, sample order and planned or plain invocation. Per level l, c_a = v_a * s_l,a, corner k: bit
 * dim-1-a -> axis a:
 *   (1) D_f[a] as in shacira_hashgrid_coords_backward; R_f = c_0 * D_f[0], then fmaf(c_a, D_f[a], R_f) for a ascending;
 *       grad_grad_output[n,l,f] = R_f (fp16: rounded once from the finished fp32 value)
 *   (3) q(kc) = (t[a1 b1 kc] - t[a1 b0 kc]) - (t[a0 b1 kc] - t[a0 b0 kc]) for the pair a < b, kc the bit of the third axis c;
 *       M_f[ab] = q (2-D), fmaf(q(1), frac_c, q(0) * (1 - frac_c)) (3-D);
 *       P[ab] = g_0 * M_0[ab], then fmaf(g_f, M_f[ab], P[ab]) for f ascending;
 *       inner[b] = c_a * P[ab] for the first a != b, then fmaf(c_a, P[ab], inner[b]) for the next (a ascending);
 *       grad[b] = 0, then fmaf(s_l,b, inner[b], grad[b]) for l ascending
 * (2) sums with float atomics and is reproducible only to the bar of shacira_hashgrid_backward.
 *
 * Table dtypes: fp32 and fp16 (values widened, grad_output read as half, grad_grad_output written as half, grad_codebook
 * accumulated in an fp32 image in the workspace and rounded once). fp64 tables are first order only: SHACIRA_EDTYPE.
 *
 *   grad_grad_coords   v, fp32 [num_coords, dim]
 *   grad_grad_output   out [num_coords, num_lods*feature_dim] of `dtype`, or NULL
 *   grad_codebook      out [table_rows, feature_dim] of `dtype`, or NULL
 *   grad_coords        out fp32 [num_coords, dim], or NULL
 *   A NULL output is not computed; at least one must be given. codebook may be NULL only when grad_codebook is the sole
 *   output, grad_output only when grad_grad_output is the sole output.
 *   plan               as for shacira_hashgrid_coords_backward
 *   workspace          shacira_hashgrid_coords_backward2_workspace_bytes(...) bytes: the fp32 image of a half table (needed only
 *                      when grad_codebook is requested), 0 for fp32 tables
 * Validation happens before any HIP call, with the codes of shacira_hashgrid_forward (SHACIRA_EWORKSPACE for a short workspace
 * or plan). num_coords == 0 returns 0 after zeroing a requested grad_codebook. No host synchronisation and no allocation: safe
 * to capture into a graph.
 */
SHACIRA_API size_t shacira_hashgrid_coords_backward2_workspace_bytes(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                                     int codebook_bitwidth, const int32_t *resolutions_host,
                                                                     int64_t table_rows, int dtype);
SHACIRA_API int shacira_hashgrid_coords_backward2(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                  int codebook_bitwidth, const int32_t *resolutions_host,
                                                  const int32_t *codebook_first_idx, int64_t table_rows, const float *coords,
                                                  const void *codebook, const void *grad_output,
                                                  const float *grad_grad_coords, int dtype, void *grad_grad_output,
                                                  void *grad_codebook, float *grad_coords, const void *plan,
                                                  size_t plan_bytes, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Triplane sampling (ABI 11, additive): TriplanarGrid (reference wisp/models/grids/triplanar_grid.py). LOD l of a call has
 * three fp32 planes fmx, fmy, fmz, each the module's NCHW parameter [1, F, S_l, S_l], S_l = 2^lods_host[l] + 1, passed as a
 * HOST array of 3 * num_lods device pointers ordered [3 * l + p] (p = 0 fmx, 1 fmy, 2 fmz; copied into the kernel arguments,
 * nothing is concatenated). fmx is read at (y, z), fmy at (x, z), fmz at (x, y): the first coordinate indexes the width (last)
 * axis. Each read is torch's grid_sample(bilinear, align_corners=True, padding_mode='reflection') in fp32, with the index
 * math of ATen/native/cuda/GridSampler.cuh:
 *   ix = ((c + 1) / 2) * (S - 1); reflected over [0, S - 1] (fabs, fmodf, flips = (int)floorf(in / span)); clipped to
 *   [0, S - 1] with fmaxf / fminf (forward: a NaN or +-inf coordinate becomes texel 0, as the device's ::max does); a value
 *   that is not finite or outside the int range becomes -100 (every corner out of bounds).
 *   corners nw (x0, y0), ne (x0+1, y0), sw (x0, y0+1), se (x0+1, y0+1), x0 = (int)floorf(ix), bounds checked per corner;
 *   weights nw = (x0+1 - ix) * (y0+1 - iy), ne = (ix - x0) * (y0+1 - iy), sw = (x0+1 - ix) * (iy - y0), se = (ix - x0) * (iy - y0).
 *   value = 0, then value += plane[c, y, x] * w for nw, ne, sw, se (in-bounds corners; separate multiply and add).
 * Output row of a sample: per LOD [x-plane F | y-plane F | z-plane F].
 *   multiscale_sum = 0 ('cat'): feats [N, num_lods * 3F], LOD-major.
 *   multiscale_sum = 1 ('sum'): feats [N, 3F], s = value_0, then s = s + value_l for l ascending.
 * Callers pass only the selected LODs (the module's 0..lod_idx).
 *
 * Backward, the derivatives of the same reads with the _set_grad twins of GridSampler.cuh: clip_coordinates_set_grad
 * gives gradient 0 at both borders (coordinate exactly -1 or +1 after reflection), reflect_coordinates_set_grad flips the
 * sign on odd reflections, a non-finite coordinate (-> -100) contributes nothing.
 *   flags & SHACIRA_TRIPLANE_GRAD_PLANES: grad_planes_host (the same layout of device pointers, each [F, S_l, S_l])
 *       overwritten with sum_n w_k(n) * g[n, l, p, c] at the four corners. The sum is accumulated with float atomics: two
 *       runs differ in the last bits. planes_host is not read.
 *   flags & SHACIRA_TRIPLANE_GRAD_COORDS: grad_coords fp32 [N, 3] overwritten (needs planes_host). Per plane, from 0,
 *       channel by channel, corners nw, ne, sw, se: gix -/+= v * (y-weight) * g, giy -/+= v * (x-weight) * g (the reference
 *       kernel's signs and order); d/du = mult_u * gix, d/dv = mult_v * giy with mult = (S - 1) / 2 * reflect sign * clip
 *       gradient; grad = 0, then += those terms for l ascending, planes x, y, z. No atomics: the same bits every run.
 *   grad_output: [N, 3F] for 'sum' (every LOD receives the same gradient), [N, num_lods * 3F] for 'cat'.
 *
 * Bounds: 1 <= num_lods <= SHACIRA_TRIPLANE_MAX_LODS, 0 <= lods_host[l] <= SHACIRA_TRIPLANE_MAX_LOD,
 * 1 <= feature_dim <= SHACIRA_TRIPLANE_MAX_FDIM, 0 <= num_coords < 2^31, coordinates fp32 [N, 3]. Validation happens before
 * any HIP call (SHACIRA_EINVAL: shapes, null pointers, flags; SHACIRA_EWORKSPACE: workspace below the query); num_coords == 0
 * writes no features (the backward still zeroes the plane gradients). No host synchronisation and no allocation: safe to
 * capture into a graph.
 */
#define SHACIRA_TRIPLANE_MAX_LODS 11
#define SHACIRA_TRIPLANE_MAX_LOD 10
#define SHACIRA_TRIPLANE_MAX_FDIM 32
#define SHACIRA_TRIPLANE_GRAD_PLANES 1
#define SHACIRA_TRIPLANE_GRAD_COORDS 2
SHACIRA_API size_t shacira_triplane_forward_workspace_bytes(int64_t num_coords, int num_lods, const int32_t *lods_host,
                                                            int feature_dim, int multiscale_sum);
SHACIRA_API int shacira_triplane_forward(int64_t num_coords, int num_lods, const int32_t *lods_host, int feature_dim,
                                         const float *coords, const float *const *planes_host, int multiscale_sum,
                                         float *feats, void *workspace, size_t workspace_bytes, void *stream);
SHACIRA_API size_t shacira_triplane_backward_workspace_bytes(int64_t num_coords, int num_lods, const int32_t *lods_host,
                                                             int feature_dim, int multiscale_sum, int flags);
SHACIRA_API int shacira_triplane_backward(int64_t num_coords, int num_lods, const int32_t *lods_host, int feature_dim,
                                          const float *coords, const float *const *planes_host, const float *grad_output,
                                          int multiscale_sum, int flags, float *const *grad_planes_host,
                                          float *grad_coords, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Octree feature lookup (ABI 11, additive): OctreeGrid / CodebookOctreeGrid (reference wisp/models/grids/octree_grid.py,
 * kaolin's unbatched_interpolate_trilinear plus the per-level glue of octree_grid.py:303-391). Level l of a call has
 *   levels_host[l]         its octree level v: G = 2^v cells and S = G + 1 lattice points per axis;
 *   tables_host[l]         fp32 [C + 1, F] row-major, C = rows_host[l] corner rows plus the reference's padding row (never
 *                          read; its gradient is zero);
 *   occupancy_host[l]      uint32 [ceil(G^3 / 32)]: bit (key & 31) of word (key >> 5), key = (x * G + y) * G + z, is set
 *                          where cell (x, y, z) is occupied;
 *   corner_index_host[l]   uint32 [ceil(S^3 / 32)][2]: per 32 lattice keys, key = (x * S + y) * S + z, {bits, rows before}:
 *                          a set bit marks a lattice point that is a corner of an occupied cell, and its table row is
 *                          rows before + popcount(bits below it). The rows are the corners in ascending key; the two z
 *                          corners of a cell edge are therefore rows r and r + 1.
 * All four are HOST arrays of num_levels entries (device pointers copied into the kernel arguments).
 *   Cell location, fp32: p = (x + 1) * (G / 2) (only the addition rounds), cell = floor(p), t = p - cell.
 *   A level contributes zeros where a component of p is not in [0, G) (a NaN or +-inf coordinate included) or the cell is
 *   unoccupied (or the index disagrees with rows_host: a row outside [0, C)). Otherwise value = sum_k w_k * row(corner k),
 *   k = 0..7 ascending, corner k = cell + (k >> 2 & 1, k >> 1 & 1, k & 1), w_k = wx * wy * wz with t or 1 - t per axis
 *   (separate multiplies and adds).
 *   multiscale_sum = 0 ('cat'): feats [N, num_levels * F], levels in the order given.
 *   multiscale_sum = 1 ('sum'): feats [N, F], s = value_0, then s = s + value_l for l ascending.
 * One launch over the samples serves every level and writes the final layout.
 *
 * Backward:
 *   flags & SHACIRA_OCTREE_GRAD_FEATURES: grad_tables_host[l] fp32 [C + 1, F] is OVERWRITTEN (zeroed by the call, padding
 *       row included) with sum_n w_k(n) * g[n, l, :] at the eight corner rows. tables_host is not read. The samples are
 *       counting-sorted by a block of cells of the finest level; a workgroup sums a block's contributions per level in LDS
 *       windows and flushes the non-zero entries with global float adds, so two runs differ in the last bits. The result
 *       does not depend on the order of the batch beyond that.
 *   flags & SHACIRA_OCTREE_GRAD_COORDS: grad_coords fp32 [N, 3] overwritten (reads tables_host):
 *       d/dx = sum_l (G_l / 2) * sum_k (dw_k / dt_x) * <row_k, g_l>, zero where the level contributes zero. A gather, one
 *       lane per sample, no atomics: the same bits every run. First order only.
 *   grad_output: [N, F] for 'sum' (every level receives the same gradient), [N, num_levels * F] for 'cat'.
 *
 * Bounds: 1 <= num_levels <= SHACIRA_OCTREE_MAX_LEVELS, 0 <= levels_host[l] <= SHACIRA_OCTREE_MAX_LEVEL,
 * 1 <= feature_dim <= SHACIRA_OCTREE_MAX_FDIM (compile-time variants for F = 1, 2, 4, 5, 8, 16; F = 5 and F = 4 are the
 * tuned cases), 0 <= rows_host[l] <= S^3, 0 <= num_coords < 2^31, coordinates fp32 [N, 3]. Validation happens before any HIP
 * call (SHACIRA_EINVAL: shapes, null pointers, flags; SHACIRA_EWORKSPACE: workspace below the query). No coordinate value
 * causes an out-of-bounds read; num_coords == 0 writes no features (the backward still zeroes the table gradients). No host
 * synchronisation and no allocation: stream-ordered and safe to capture into a graph.
 */
#define SHACIRA_OCTREE_MAX_LEVELS 11
#define SHACIRA_OCTREE_MAX_LEVEL 10
#define SHACIRA_OCTREE_MAX_FDIM 32
#define SHACIRA_OCTREE_GRAD_FEATURES 1
#define SHACIRA_OCTREE_GRAD_COORDS 2
SHACIRA_API size_t shacira_octree_forward_workspace_bytes(int64_t num_coords, int num_levels, const int32_t *levels_host,
                                                          int feature_dim, int multiscale_sum);
SHACIRA_API int shacira_octree_forward(int64_t num_coords, int num_levels, const int32_t *levels_host, int feature_dim,
                                       const float *coords, const float *const *tables_host, const int64_t *rows_host,
                                       const void *const *corner_index_host, const void *const *occupancy_host,
                                       int multiscale_sum, float *feats, void *workspace, size_t workspace_bytes,
                                       void *stream);
SHACIRA_API size_t shacira_octree_backward_workspace_bytes(int64_t num_coords, int num_levels, const int32_t *levels_host,
                                                           int feature_dim, int multiscale_sum, int flags);
SHACIRA_API int shacira_octree_backward(int64_t num_coords, int num_levels, const int32_t *levels_host, int feature_dim,
                                        const float *coords, const float *const *tables_host, const int64_t *rows_host,
                                        const void *const *corner_index_host, const void *const *occupancy_host,
                                        const float *grad_output, int multiscale_sum, int flags,
                                        float *const *grad_tables_host, float *grad_coords, void *workspace,
                                        size_t workspace_bytes, void *stream);

/*
 * Mesh to signed distance (ABI 11, additive): the reference's `mesh_to_sdf_cuda` (wisp/ops/mesh/compute_sdf.py; kernels
 * kernel_mesh2sdf_quad + kernel_quad_aggr of wisp/csrc/external/mesh2sdf_kernel.cu): for every point the distance to the
 * nearest non-degenerate triangle, negative where the point is inside by 13-direction ray stabbing. Brute force over the
 * N x T pairs.
 *
 *   points     [N, 3] fp32
 *   triangles  [T, 3, 3] fp32: the vertices a, b, c of every triangle (V[F])
 *   sdf        out, [N] fp32
 *
 * All arithmetic is fp32, evaluated WITHOUT contraction (the library is built with -ffp-contract=off -fno-fast-math), in
 * these fixed shapes:
 *   dot(x, y)   = (x0*y0 + x1*y1) + x2*y2
 *   cross(x, y) = (x1*y2 - x2*y1, x2*y0 - x0*y2, x0*y1 - x1*y0)
 *   |t|^2       = (t0*t0 + t1*t1) + t2*t2
 *   sgn(x)      = copysignf(1, x);   clamp01(x) = fmaxf(0, fminf(x, 1));   reciprocals are IEEE 1.0f / x
 * Per triangle:
 *   e0 = b - a, e1 = c - b, e2 = a - c;  n = cross(e0, e2);  m_i = cross(e_i, n);  r_i = 1 / dot(e_i, e_i);
 *   r_n = 1 / dot(n, n);  g = -e2
 * Per (point p, triangle) pair:  p0 = p - a, p1 = p - b, p2 = p - c.
 * Distance, only for triangles with a non-zero n (any component != 0):
 *   s = (sgn(dot(m0, p0)) + sgn(dot(m1, p1))) + sgn(dot(m2, p2))
 *   s < 2:      d2 = fminf(E0, fminf(E1, E2)),  E_i = |e_i * clamp01(dot(e_i, p_i) * r_i) - p_i|^2
 *               (component-wise t_k = e_ik * x - p_ik)
 *   otherwise:  d2 = (dot(n, p0) * dot(n, p0)) * r_n
 *   a negative d2 becomes 0;  m = fminf of d2 over all such triangles, +inf if there are none.
 * Ray stabbing, for EVERY triangle (degenerate ones included):
 *   q = cross(p0, e0);  tau = dot(g, q)
 *   the 13 directions, in this order, h = 0.707106781f, k = 0.577350269f:
 *     (1,0,0) (0,1,0) (0,0,1)  (0,h,h) (h,0,h) (h,h,0)  (0,h,-h) (h,0,-h) (h,-h,0)  (k,k,k) (-k,k,k) (k,-k,k) (k,k,-k)
 *   per direction dir:  w = cross(dir, g);  det = dot(e0, w);  skipped when -1e-8 < det < 1e-8 (det widened to double and
 *     compared with the double constants: (float)1e-8 is a different threshold);  inv = 1 / det;
 *     u = dot(p0, w) * inv, skipped if u < 0 or u > 1;   v = dot(dir, q) * inv, skipped if v < 0 or u + v > 1;
 *     t = tau * inv:  t >= 0 sets pos[dir], otherwise neg[dir].
 * Result:  dist = sqrtf(m);  the point is inside iff every one of the 13 directions has both pos and neg set;
 *          sdf = inside ? -dist : dist.
 * T == 0 gives +inf everywhere. Non-finite points or vertices do not fault; their outputs are unspecified.
 *
 * The minimum and the 26 flags are order-free and every other value is a function of one triangle or of one (point,
 * triangle) pair: any partition of the triangles over lanes, workgroups or passes gives the same bits, and so does
 * precomputing the per-triangle and per-(triangle, direction) quantities. (The kernels leave out the terms of dot(dir, q) whose
 * direction component is a literal 0: for finite inputs that changes at most the sign of a zero, which no comparison above
 * sees.) nvcc contracts by default, so the reference's own bits can differ in the last place; the contract is the uncontracted
 * sequence, the position the hash-grid oracle's mode 0 takes.
 *
 *   workspace  shacira_mesh_sdf_workspace_bytes(N, T) bytes, 16-byte aligned: the per-triangle records of ONE pass (the
 *              triangles are processed in passes of SHACIRA_MESH_SDF_PASS_TRIANGLES, so at most that many records of 352
 *              bytes: 5.5 MiB whatever T) plus 8 bytes per point (minimum and flags, merged across triangle chunks with one
 *              atomicMin and one atomicOr per point and chunk). 0 when N == 0 or T == 0 (workspace may then be NULL). The call
 *              initialises everything it reads from it: stale contents do not matter. Within a pass a workgroup row walks
 *              a chunk of triangles whose length is a multiple of SHACIRA_MESH_SDF_CHUNK_GRANULE; the number of chunks is
 *              chosen from N and T (small N: enough chunks to fill the chip; large N: one).
 * Bounds: 0 <= N, T < 2^31. Validation happens before any HIP call: negative or too large counts and NULL operands return
 * SHACIRA_EINVAL, a workspace below the query SHACIRA_EWORKSPACE; N == 0 returns 0 and launches nothing; T == 0 fills +inf.
 * Everything runs on `stream`; no host synchronisation and no allocation: safe to capture into a graph.
 */
#define SHACIRA_MESH_SDF_PASS_TRIANGLES 16384
#define SHACIRA_MESH_SDF_CHUNK_GRANULE 32
SHACIRA_API size_t shacira_mesh_sdf_workspace_bytes(int64_t num_points, int64_t num_triangles);
SHACIRA_API int shacira_mesh_sdf(int64_t num_points, int64_t num_triangles, const float *points, const float *triangles,
                                 float *sdf, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Closest point on a mesh (ABI 11, additive): shacira_mesh_sdf keeping the winner. One pass over the N x T pairs gives the
 * distance, the closest point and the index of the triangle it lies on (the reference's wisp/ops/mesh/closest_point.py is an
 * `assert False`; closest_tex.py builds on it).
 *
 *   points     [N, 3] fp32
 *   triangles  [T, 3, 3] fp32
 *   flags      SHACIRA_MESH_CLOSEST_SIGNED: dist is negative inside (13-direction ray stabbing); any other bit: SHACIRA_EINVAL
 *   dist       out, [N] fp32
 *   hit        out, [N, 3] fp32: the closest point
 *   tidx       out, [N] int32: the triangle it lies on, -1 if there is none
 *
 * Symbols, shapes and rounding are those of the shacira_mesh_sdf contract above. Per pair, d2 is exactly its d2 (a negative
 * d2 becomes +0); only triangles with a non-zero n are candidates.
 * Winner:  the candidate with the least d2; among equal d2 the lowest triangle index, counted over the whole mesh. A NaN d2
 *          never wins (and neither does +inf): walking ascending indices from best = +inf, "replace iff d2 < best".
 * dist:    sqrtf(d2 of the winner); with SIGNED negated where all 13 directions have both stab flags set, by the rule above.
 *          So dist has the bits of shacira_mesh_sdf's sdf when SIGNED and of its absolute value otherwise. Without SIGNED
 *          the stabbing is not executed at all.
 * hit:     once per point, from the winning triangle:
 *            s, x_i = clamp01(dot(e_i, p_i) * r_i) and E_i as above
 *            s >= 2:     k = dot(n, p0) * r_n;  hit_j = p_j - n_j * k
 *            otherwise:  i* = 0 if E0 <= E1 && E0 <= E2, else 1 if E1 <= E2, else 2;
 *                        hit_j = v_{i*,j} + e_{i*,j} * x_{i*}   with v_0 = a, v_1 = b, v_2 = c
 * No candidate (T == 0, or every triangle degenerate):  dist = +inf, tidx = -1, hit = p.
 *
 * The argmin with its tie rule, the minimum and the 26 flags are order-free and every other value is a function of one
 * triangle or of one (point, triangle) pair: any partition of the triangles over lanes, chunks or passes gives the same bits.
 * (Chunks are merged with one 64-bit atomicMin per point and chunk on (bits(d2) << 32) | index: non-negative floats order
 * like their bits, and the low word is the tie rule.)
 *
 *   workspace  shacira_mesh_closest_workspace_bytes(N, T, flags) bytes, 16-byte aligned: the records of one pass, as for
 *              shacira_mesh_sdf, plus 16 bytes per point (key, flags). 0 when N == 0 or the arguments are invalid. The call
 *              initialises everything it reads from it.
 * Bounds and validation as for shacira_mesh_sdf: 0 <= N, T < 2^31; negative or too large counts, unknown flag bits and NULL
 * operands return SHACIRA_EINVAL and a workspace below the query SHACIRA_EWORKSPACE, all before any HIP call; N == 0 returns
 * 0 and launches nothing. Everything runs on `stream`; no host synchronisation and no allocation: safe to capture.
 */
#define SHACIRA_MESH_CLOSEST_SIGNED 1
SHACIRA_API size_t shacira_mesh_closest_workspace_bytes(int64_t num_points, int64_t num_triangles, int32_t flags);
SHACIRA_API int shacira_mesh_closest(int64_t num_points, int64_t num_triangles, const float *points, const float *triangles,
                                     int32_t flags, float *dist, float *hit, int32_t *tidx, void *workspace,
                                     size_t workspace_bytes, void *stream);

/*
 * Mesh to occupancy (ABI 11, additive): the triangles rasterised into the dense occupancy of one octree level. The reference
 * gets there by sampling (wisp/ops/spc/conversions.py mesh_to_octree: surface samples plus a copy jittered by
 * +-1 / 2^(level + 1) in cube coordinates, a quarter of a cell, both quantised); this call computes such a set exactly and
 * deterministically. The limit of the reference's sampling is the set of margin 0.25 (a jittered sample lies within 0.75 cell,
 * per axis, of the centre of its cell); a larger margin gives a superset of it.
 *
 *   triangles        [T, 3, 3] fp32, the layout of shacira_mesh_sdf, in the cube's coordinates [-1, 1]^3
 *   level            0 <= level <= SHACIRA_OCTREE_MAX_LEVEL (the bound of the dense grids of the ray kernels, too); G = 2^level
 *   margin           fp32, finite, >= 0, in cells
 *   occupancy_words  out, uint32 [ceil(G^3 / 32)]: bit (key & 31) of word (key >> 5), key = (x * G + y) * G + z -- the
 *                    occupancy_host layout of shacira_octree_forward
 *   occupancy_grid   out, may be NULL: uint8 [G][G][G] indexed [x][y][z], 1 where the bit is set, 0 elsewhere (what the ray
 *                    kernels and OctreeAS.occupancy_grid hold); expanded from the words by a finishing kernel; 16-byte aligned
 * Both outputs are overwritten (zeroed by the call).
 *
 * The set: cell (i, j, k) is set iff some valid triangle overlaps the CLOSED cube with centre (i + .5, j + .5, k + .5) and
 * half-extent H = 0.5 + margin, both in grid units g = (v + 1) * (G / 2): the 13-axis separating-axis test (three cube axes,
 * the triangle normal, nine edge x axis cross products) in its projected form -- an integer bounding box, the plane slab and
 * three 2-D edge-function triples -- with closed comparisons throughout: touching counts. All arithmetic is fp32 without
 * contraction, one rounding per operator, cross(x, y) as in the shacira_mesh_sdf contract, in these fixed shapes:
 * Per triangle (a, b, c as given):
 *   valid  iff  cross(b - a, a - c) has a non-zero component (the record flag of shacira_mesh_sdf, on the vertices as given)
 *          and all nine grid-unit coordinates are finite. An invalid triangle marks nothing.
 *   A = (a + 1) * (G / 2), B, C alike (component-wise; G / 2 is exact, 0.5 at level 0);  H = 0.5f + margin
 *   E0 = B - A, E1 = C - B, E2 = A - C;  N = cross(E0, E1);  rN = H * ((|Nx| + |Ny|) + |Nz|)
 *   cube axes, per axis c:  lo_c = fmaxf(ceilf((fminf(fminf(A_c, B_c), C_c) - H) - 0.5f), 0)
 *                           hi_c = fminf(floorf((fmaxf(fmaxf(A_c, B_c), C_c) + H) - 0.5f), G - 1)
 *          cell index i passes iff lo_c <= i <= hi_c: the integers with i + 0.5 in [min - H, max + H], CLIPPED to the grid.
 *          Geometry outside the cube therefore marks nothing (a stated deviation: the reference clamps outside samples into
 *          the border cells).
 *   projection k = 0, 1, 2 drops axis k: (u, v) = (y, z), (z, x), (x, y);  sigma_k = N_k >= 0 ? +1 : -1;
 *          edge i = 0, 1, 2 starts at P_i = A, B, C:  mu = -sigma_k * E_i[v],  mv = sigma_k * E_i[u]  (exact),
 *          r = H * (|mu| + |mv|)
 * Per (cell, triangle) pair, centre p = (i + .5, j + .5, k + .5) (exact):
 *   plane     s = (Nx * (px - Ax) + Ny * (py - Ay)) + Nz * (pz - Az);   passes iff  -rN <= s  and  s <= rN
 *   edges     f = (mu * (p_u - P_i[u]) + mv * (p_v - P_i[v])) + r;      passes iff  f >= 0      (all nine)
 * A NaN in any of these (overflowing products of far-away vertices) fails its comparison and the pair marks nothing.
 * With sigma from the sign of N_k, a projection that degenerates to a segment (N_k == 0) still gives the slab around that
 * segment, which is what the three edge x axis products of that projection test.
 *
 * The predicate belongs to one (cell, triangle) pair and the combine is an OR: any split of the work over passes, workgroups
 * and lanes gives the same bits, and two calls give identical outputs. The call splits it into COLUMN WORDS -- one (x, y)
 * column of a triangle's bounding box crossed with one 32-bit word of its z range -- one lane and at most one atomicOr each,
 * lanes found by binary search in the exclusive scan of the per-triangle unit counts. tests/mesh_voxelize_ref.py restates
 * the formulas in numpy and reproduces the cell set exactly.
 *
 *   workspace  shacira_mesh_voxelize_workspace_bytes(T, level) bytes, 16-byte aligned: the 192-byte records and the 64-bit
 *              unit offsets of ONE pass of at most SHACIRA_MESH_VOXELIZE_PASS_TRIANGLES triangles (6.25 MiB whatever T).
 *              0 when T == 0 (workspace may then be NULL) or the arguments are invalid. The call initialises what it reads.
 * Bounds: 0 <= T < 2^31. Validation happens before any HIP call: a bad count, level or margin (negative, NaN, infinite) and
 * NULL or misaligned operands return SHACIRA_EINVAL, a workspace below the query SHACIRA_EWORKSPACE. T == 0 zeroes the outputs.
 * Everything runs on `stream`, which the call SYNCHRONISES once per pass (the host reads the pass's unit count to size the
 * launch): not capturable into a graph, unlike shacira_mesh_sdf. No allocation.
 */
#define SHACIRA_MESH_VOXELIZE_PASS_TRIANGLES 32768
SHACIRA_API size_t shacira_mesh_voxelize_workspace_bytes(int64_t num_triangles, int level);
SHACIRA_API int shacira_mesh_voxelize(int64_t num_triangles, const float *triangles, int level, float margin,
                                      uint32_t *occupancy_words, uint8_t *occupancy_grid, void *workspace,
                                      size_t workspace_bytes, void *stream);

/*
 * Mesh point sampling (ABI 11, additive): training points on a mesh, near it, in the cube or inside octree cells, every one
 * a pure function of (seed, sample index), optionally only those inside the occupied cells of one octree level. The
 * reference samples with a chain of host-side torch calls on the global generator (wisp.ops.mesh sample_surface,
 * sample_near_surface, sample_uniform and wisp.ops.spc sample_spc) and filters with cat, query and a boolean
 * index (wisp/datasets/formats/octree_sdf_dataset.py); here one device function, make_sample(i), serves a counting and a
 * writing kernel. tests/mesh_sample_ref.py restates it in numpy.
 *
 *   mode             SHACIRA_MESH_SAMPLE_SURFACE / NEAR / CUBE / CELLS
 *   n                samples, local indices i = 0 .. n - 1
 *   index_base       >= 0; the counter of sample i is idx = index_base + i (int64)
 *   seed, segment    the Philox key and the fourth counter word (the datasets: the technique's position in sample_mode)
 *   words            may be NULL. uint32 [n, 8]: row i replaces the eight Philox words of sample i (words 0..3 draw 0,
 *                    4..7 draw 1), e.g. a low-discrepancy sequence. seed, segment and index_base are then not used
 *   num_triangles T, triangles [T, 3, 3] fp32 (the layout of shacira_mesh_sdf), cdf uint32 [T]    SURFACE and NEAR: T >= 1
 *   sigma            NEAR: the displacement's standard deviation (the reference's misnamed `variance`)
 *   num_cells C, corners int16 [C, 3] (the layout of OctreeAS.points), samples_per_cell >= 1, cell_level    CELLS only:
 *                    n must equal C * samples_per_cell, 0 <= cell_level <= SHACIRA_OCTREE_MAX_LEVEL
 *   occupancy_words  may be NULL (no filter). uint32 [ceil(G^3 / 32)], G = 2^occupancy_level, 0 <= occupancy_level <=
 *                    SHACIRA_OCTREE_MAX_LEVEL: bit (key & 31) of word (key >> 5), key = (x * G + y) * G + z -- what
 *                    shacira_mesh_voxelize writes and OctreeAS.packed_occupancy returns
 * Operands of other modes are not read and may be NULL.
 *
 * Random words: Philox4x32-10 (Salmon et al. 2011; multipliers D2511F53, CD9E8D57, key increments 9E3779B9, BB67AE85).
 *   key = (seed low word, seed high word);  counter = (idx low word, idx high word, draw, segment)
 *   draw 0 gives w0..w3 (the face and barycentric words, or the three coordinates of CUBE and CELLS; w3 is unused),
 *   draw 1 gives g0..g3 (the Gaussian words; evaluated by NEAR only).
 *   U(w) = (float)(w >> 8) * 2^-24 in [0, 1);   U1(w) = (float)((w >> 8) + 1) * 2^-24 in (0, 1]   (both exact)
 * Face of a word (SURFACE, NEAR): cdf is the inclusive integer CDF of the face areas, non-decreasing, cdf[T - 1] > 0
 *   (shacira_amd.hip_ops.mesh_face_cdf: a, b, c fp32; x = a - b, y = b - c in fp32; cross(x, y), its squares and their sum
 *   ((nx^2 + ny^2) + nz^2), the square root and the running sum in fp64, in index order;
 *   cdf[t] = min(floor(sum[t] / sum[T - 1] * 2^32), 2^32 - 1)). The rule, integers only:
 *       w' = min(w0, cdf[T - 1] - 1);   face = the FIRST t with cdf[t] > w'   (a binary search for the upper bound)
 *   Face t thus owns the words [cdf[t - 1], cdf[t]) (cdf[-1] = 0) and the last face of positive width also those from
 *   cdf[T - 1] up. So: a face of zero area (cdf[t] == cdf[t - 1]; first: cdf[0] == 0) owns no word, wherever it stands;
 *   every word has a face, since cdf[T - 1] > w'; and the share of a face differs from its area share by less than 2^-32 from
 *   the floors at its two ends (no word is lost to the clamp). A cdf that breaks the preconditions reads nothing out of
 *   bounds: the search never leaves [0, T - 1].
 * Points, fp32, no contraction, one rounding per operator, cross(x, y) as in the shacira_mesh_sdf contract:
 *   SURFACE  u = sqrtf(U(w1)), v = U(w2);  p = ((1 - u) * a + (u * (1 - v)) * b) + (u * v) * c  per coordinate;
 *            normal = cross(a - b, b - c), not normalised;  face index = t
 *   NEAR     the SURFACE point of (w0, w1, w2), then p_k = p_k + sigma * n_k with Box-Muller normals:
 *            r = sqrtf(-2 * logf(U1(g0))), r' = sqrtf(-2 * logf(U1(g2)));  (s, c) = sincospif(2 * U(g1)), c' = cospi(2 * U(g3))
 *            (the arguments are exact);  n = (r * c, r * s, r' * c').  sigma == 0 gives the SURFACE point. logf and
 *            sincospif are the device library's: tests/test_gpu_mesh_sample.py bounds them against fp64
 *   CUBE     p_k = U(w_k) * 2 - 1
 *   CELLS    cell = i / samples_per_cell, c = corners[cell], W = 2 / 2^cell_level:  p_k = (c_k * W - 1) + U(w_k) * W
 *            normal = 0 and face index = -1 for CUBE and CELLS
 * Filter (occupancy_words != NULL): a sample is kept iff OctreeAS.query gives pidx > -1 at that level:
 *   q_k = floorf((G * (p_k + 1)) / 2) in fp32;  kept iff 0 <= q_k < G for every k (false for NaN) and the bit of key(q) is set.
 *
 * shacira_mesh_sample_count: occupancy_words required. block_counts int32 [ceil(n / SHACIRA_MESH_SAMPLE_BLOCK)]: how many of
 *   the block's consecutive indices are kept. One launch, no host synchronisation.
 * shacira_mesh_sample: points fp32 [rows, 3]; normals fp32 [rows, 3], face_idx int32 [rows], source_idx int64 [rows] (the
 *   local index i) may each be NULL.
 *   block_offsets == NULL (occupancy_words must be NULL too): rows = n, sample i goes to row i.
 *   block_offsets int64 [ceil(n / 256)], the exclusive scan of block_counts (occupancy_words required): the kept samples of
 *   block b go to rows block_offsets[b] + rank, the rank counted in index order among the kept samples of the block (wavefront
 *   ballot plus a four-entry LDS prefix): the output is the kept subsequence, in order. The samples are made again from their
 *   indices, so no intermediate array exists and the two launches cannot disagree.
 * One thread per sample, workgroups of 256, no scratch, no workspace, no allocation; all stores are ordinary vector stores.
 *
 * Bounds: 0 <= n, T, C < 2^31; index_base + n does not overflow int64. Address arithmetic is 64-bit. Validation happens
 * before any HIP call: an unknown mode, bad counts or levels, n != C * samples_per_cell, and NULL operands of the mode return
 * SHACIRA_EINVAL; n == 0 returns 0 and launches nothing. Each call is ONE launch on `stream` with no host synchronisation:
 * safe to capture into a graph. The filtered form as a whole (count, scan, read the total to size the outputs, write) is
 * not capturable: the caller reads the total back between the two calls.
 */
#define SHACIRA_MESH_SAMPLE_SURFACE 0
#define SHACIRA_MESH_SAMPLE_NEAR 1
#define SHACIRA_MESH_SAMPLE_CUBE 2
#define SHACIRA_MESH_SAMPLE_CELLS 3
#define SHACIRA_MESH_SAMPLE_BLOCK 256
SHACIRA_API int shacira_mesh_sample_count(int mode, int64_t n, int64_t index_base, uint64_t seed, uint32_t segment,
                                          const uint32_t *words, int64_t num_triangles, const float *triangles,
                                          const uint32_t *cdf, float sigma, int64_t num_cells, const int16_t *corners,
                                          int samples_per_cell, int cell_level, const uint32_t *occupancy_words,
                                          int occupancy_level, int32_t *block_counts, void *stream);
SHACIRA_API int shacira_mesh_sample(int mode, int64_t n, int64_t index_base, uint64_t seed, uint32_t segment,
                                    const uint32_t *words, int64_t num_triangles, const float *triangles,
                                    const uint32_t *cdf, float sigma, int64_t num_cells, const int16_t *corners,
                                    int samples_per_cell, int cell_level, const uint32_t *occupancy_words,
                                    int occupancy_level, const int64_t *block_offsets, float *points, float *normals,
                                    int32_t *face_idx, int64_t *source_idx, void *stream);

/*
 * Structural similarity (SSIM) of a prediction x against a target y, and its gradient with respect to x: what
 * skimage.metrics.structural_similarity(x, y, data_range=R, gaussian_weights=True, sigma=1.5, channel_axis=2) computes, the
 * second number the reference reports per validation image (wisp/ops/image/metrics.py:111-132).
 *   x, y          [H, W, pixel_stride] fp32, channels last; the first `channels` floats of every pixel are read. A
 *                 pixel_stride above `channels` lets the RGB of an RGBA buffer through without a copy
 *   data_range    R, fp32, finite, > 0
 *   value         out, ONE fp64: the SSIM (overwritten)
 *   map           out, may be NULL: fp32 [H, W, channels], the score of every pixel (overwritten)
 *   grad          backward: ONE fp32 on the device, dL/d(value)
 *   grad_x        backward out: fp32 [H, W, pixel_stride] (overwritten; channels >= `channels` receive exactly zero).
 *                 There is no gradient with respect to y.
 *
 * Per channel, on the planes x, y:
 *   window   w[k] = exp(-0.5 (k / 1.5)^2), k = -5 .. 5, divided by their sum in fp64, then rounded to fp32; G = the window along
 *            each axis (rows first). The weights from the edge inwards:
 *            0.00102838, 0.00759876, 0.03600077, 0.10936069, 0.21300554, 0.26601172
 *   fields   ux = G x, uy = G y, uxx = G(x x), uyy = G(y y), uxy = G(x y);  cov = 121 / 120
 *            vx = cov (uxx - ux ux), vy = cov (uyy - uy uy), vxy = cov (uxy - ux uy)
 *   score    C1 = (0.01 R)^2, C2 = (0.03 R)^2
 *            S = ((2 ux uy + C1) (2 vxy + C2)) / ((ux^2 + uy^2 + C1) (vx + vy + C2))
 *   value    the mean of S over the (H - 10)(W - 10) VALID pixels -- at least 5 away from every border, so only windows that
 *            lie wholly inside the image count -- accumulated in fp64; then the plain mean over the channels
 *   borders  only the map sees them: G there reads the image through scipy's mode='reflect' (d c b a | a b c d | d c b a)
 * The fields are taken of x - mx and y - my, one shift per (tile, channel) -- the median of the means of three rows of the tile
 * (its centre row and the rows two and four above it, over the tile's columns and its left halo), so that no single pixel
 * decides it; 0 when that is not finite -- and the shift is added back to ux and uy: vx, vy and vxy do not change under a shift, but on a nearly flat image the
 * cancellation in uxx - ux ux then leaves the differences of neighbouring pixels and not the rounding of their squares.
 * All arithmetic is fp32, one rounding per operator, except the window's taps, which are fused multiply-adds, summed from the
 * outer pair inwards: w5 (v[-5] + v[5]), then fma(w4, v[-4] + v[4], .), ..., the centre last. With x == y every S is exactly 1
 * and so is the value. A NaN pixel makes the value NaN and the map NaN in its 11 x 11 neighbourhood; nothing is clamped.
 *
 * Backward: with L = grad * value, per valid pixel q (zero elsewhere), A1, A2 the numerator's factors and B1, B2 the
 * denominator's, P = A1 / B1, Q = A2 / B2:
 *   dS/dux  = 2 (uy Q - ux S) / B1 + 2 cov (ux S - uy P) / B2       dS/duxx = -cov S / B2       dS/duxy = 2 cov P / B2
 *   grad_x  = (grad / (channels (H - 10)(W - 10))) * (Gt[dS/dux] + 2 x Gt[dS/duxx] + y Gt[dS/duxy])
 * Gt is the transpose of the valid filter: the same window over the three fields with zeros outside the valid region. At
 * x == y the three terms cancel to the bit: grad_x is exactly zero. The fields are recomputed, nothing is kept from a forward.
 *
 * One workgroup per (tile of SHACIRA_SSIM_TILE_H x SHACIRA_SSIM_TILE_W pixels, channel), tiles counted from pixel (0, 0).
 * Reduction order: a tile's valid scores are added in fp64 by lane shuffles and then over its four waves; a one-workgroup
 * finishing kernel adds the partials of a channel (thread t the tiles t, t + 1024, ..., then a binary tree over the threads),
 * divides by the valid pixels and averages the channels. No floating-point atomics: two calls on the same operands return the
 * same bits in value, map and grad_x.
 *
 *   workspace  shacira_ssim_workspace_bytes(H, W, channels, backward) bytes, 16-byte aligned. Forward (backward == 0): one
 *              fp64 partial per (channel, tile). Backward: the three derivative planes, 3 * channels * H * W fp32. 0 when
 *              the arguments are invalid. The call initialises what it reads.
 * Bounds: H, W >= SHACIRA_SSIM_WINDOW (skimage raises below it), 1 <= channels <= pixel_stride <= 65535, at most 2^31 - 1
 * tiles; all index arithmetic is 64-bit (a gigapixel image is in range). Validation happens before any HIP call: a bad size,
 * channel count or data_range and NULL x, y, value, grad or grad_x return SHACIRA_EINVAL and nothing is enqueued; a workspace
 * below the query returns SHACIRA_EWORKSPACE. Everything runs on `stream`: no synchronisation, no allocation, capturable.
 */
#define SHACIRA_SSIM_WINDOW 11
#define SHACIRA_SSIM_TILE_H 16
#define SHACIRA_SSIM_TILE_W 64
SHACIRA_API size_t shacira_ssim_workspace_bytes(int64_t height, int64_t width, int channels, int backward);
SHACIRA_API int shacira_ssim_forward(int64_t height, int64_t width, int pixel_stride, int channels, const float *x,
                                     const float *y, float data_range, double *value, float *map, void *workspace,
                                     size_t workspace_bytes, void *stream);
SHACIRA_API int shacira_ssim_backward(int64_t height, int64_t width, int pixel_stride, int channels, const float *x,
                                      const float *y, float data_range, const float *grad, float *grad_x, void *workspace,
                                      size_t workspace_bytes, void *stream);

/*
 * Positional-encoding rows: the decoder MLP's input [prefix | coords | sin | cos] written by one kernel, what
 * torch.cat([prefix, PositionalEmbedder(coords)], -1) builds from seven (wisp/models/embedders/positional_embedder.py:60-66,
 * wisp/models/nefs/image.py:146-148). All operands fp32; every stride counts floats between the starts of two rows.
 *   n              rows; 0 returns 0 with nothing enqueued, whatever the pointers and strides (d, num_bands and prefix_width
 *                  are checked first)
 *   d              coordinates per row, 1 .. SHACIRA_POSENC_MAX_DIM
 *   num_bands      F, 1 .. SHACIRA_POSENC_MAX_BANDS; bands[F] on the device, any values (linear sampling gives non-powers of two)
 *   include_input  non-zero: the coordinates are part of the row, I = d; zero: I = 0
 *   prefix_width   P, 0 .. SHACIRA_POSENC_MAX_PREFIX; prefix [n, P] may be NULL when P == 0
 *   E = I + 2 d F, the row is P + E wide:
 *     col 0 .. P-1              prefix, copied bit for bit
 *     col P .. P+I-1            coords, copied bit for bit (-0.0, Inf and NaN payloads included)
 *     col P+I + k*d + j         sin(a_kj)       a_kj = coords[j] * bands[k], ONE fp32 multiply
 *     col P+I + d*F + k*d + j   cos(a_kj)       both from the device library's sincosf (full-range reduction; a non-finite
 *                                               a_kj gives NaN in both columns)
 *   out            [n, >= P+E] with out_stride >= P+E; columns beyond P+E are not written
 * shacira_posenc_backward: the gradient with respect to the coordinates from the SAVED row of the forward (`row`, any
 * row_stride >= P+E; only its sin / cos columns are read) and grad_out (same layout, own stride); no trigonometry, the
 * coordinates are not needed. grad_coords [n, d] dense, overwritten:
 *     gc_j = [I > 0] g_in_j + sum_k bands[k] * (cos_kj * g_sin_kj - sin_kj * g_cos_kj)
 * fp32, one rounding per operator, the terms added in k order onto g_in_j (onto 0 without it). The gradient with respect to
 * the prefix is grad_out[:, :P] itself: no kernel.
 * shacira_posenc_backward2: the backward of that call. With gg [n, d] dense = dL/d(grad_coords) it overwrites two dense
 * [n, P+E] arrays:
 *     grad_row        sin col: -(b_k g_cos_kj) gg_j     cos col: +(b_k g_sin_kj) gg_j     every other column: 0
 *     grad_grad_out   sin col: +(b_k cos_kj) gg_j       cos col: -(b_k sin_kj) gg_j       input col j: gg_j     prefix: 0
 * grad_row is a gradient with respect to the forward's OUTPUT: sent through shacira_posenc_backward once more it yields the
 * -sum_k b_k^2 (...) term of the second derivative with respect to the coordinates.
 *
 * Pointers need the 4-byte alignment of a float only; when P is a multiple of 4 and prefix, out and their strides are multiples
 * of 16 bytes the prefix moves 16 bytes at a time, with the same result. Validation precedes any HIP call: n < 0, d, num_bands
 * or prefix_width out of range, a NULL operand (prefix only when P > 0), out_stride / row_stride / grad_stride < P+E,
 * coords_stride < d, prefix_stride < P, or n * stride beyond 2^59 return SHACIRA_EINVAL and nothing is enqueued. No workspace,
 * no allocation, no synchronisation, no atomics: everything runs on `stream`, is capturable, and two calls on the same operands
 * return the same bits.
 */
#define SHACIRA_POSENC_MAX_DIM 4
#define SHACIRA_POSENC_MAX_BANDS 64
#define SHACIRA_POSENC_MAX_PREFIX (1 << 30)
SHACIRA_API int shacira_posenc_forward(int64_t n, int d, int num_bands, int include_input, int64_t prefix_width,
                                       const float *coords, int64_t coords_stride, const float *prefix, int64_t prefix_stride,
                                       const float *bands, float *out, int64_t out_stride, void *stream);
SHACIRA_API int shacira_posenc_backward(int64_t n, int d, int num_bands, int include_input, int64_t prefix_width,
                                        const float *row, int64_t row_stride, const float *grad_out, int64_t grad_stride,
                                        const float *bands, float *grad_coords, void *stream);
SHACIRA_API int shacira_posenc_backward2(int64_t n, int d, int num_bands, int include_input, int64_t prefix_width,
                                         const float *gg, const float *row, int64_t row_stride, const float *grad_out,
                                         int64_t grad_stride, const float *bands, float *grad_row, float *grad_grad_out,
                                         void *stream);

/*
 * Ray generation: origins, unit directions and composited target colours of n (view, pixel) pairs in one kernel, from one
 * small record per camera and the uint8 training images -- what wisp/ops/raygen/raygen.py:46-119 computes per view and
 * wisp/datasets/formats/nerf_standard_dataset.py:407-428 stores for every pixel of every view. Not differentiable.
 *   cams           fp32 [num_views, SHACIRA_RAYGEN_RECORD_FLOATS] on the device, 16-byte aligned; one record, rounded from the
 *                  fp64 camera:
 *                     0 ..  8   R, the camera-to-world rotation, row-major (the transpose of the view matrix's 3x3)
 *                     9 .. 11   t, the camera's position in the world
 *                    12, 13     tan of half the horizontal / vertical field of view: W / (2 fx), H / (2 fy)
 *                    14, 15     x0, y0: the principal point as an offset in pixels from the image centre
 *                    16         lens: 0 pinhole, anything else orthographic
 *                    17, 18     fov_distance * (W / H), fov_distance (orthographic lens)
 *                    19         reserved, 0
 *   width, height  W, H of every view, both > 0, W * H < 2^31
 *   view_idx, pixel_idx   int32 [n], pixel = y * W + x. Both NULL: the whole-view form, ray i is pixel i mod (H W) of view
 *                  i div (H W) and n <= num_views * H * W
 *   jitter         fp32 [n, 2] (jx, jy), 8-byte aligned, or NULL: a sub-pixel offset added to the pixel centre
 *   images         uint8 [num_views, H, W, channels], channels 3 or 4; NULL: rgb and mask are not written (and may be NULL)
 *   bg_mode        SHACIRA_RAYGEN_BG_WHITE / _BLACK: what a 4-channel image is composited over
 *   origins, dirs, rgb   fp32 [n, 3] dense; mask uint8 [n], 0 or 1
 * fp32, one rounding per operator, in this order (correctly rounded / and sqrt, no fused multiply-add):
 *     px = ((x + 0.5) + jx) - x0        py = ((y + 0.5) + jy) + y0        (the orthographic lens skips x0 and y0, as the
 *     u  = 2 (px / W) - 1               v  = 2 (py / H) - 1                reference's generate_ortho_rays does)
 *     pinhole        d_cam = (u tanx, -v tany, -1)       origin = t, the record's bits
 *     orthographic   d_cam = (0, 0, -1)                  o_cam = (u fd aspect, -v fd, 0),  origin_i = (R_i0 o_x + R_i1 o_y) + t_i
 *     w_i = (R_i0 d_x + R_i1 d_y) + R_i2 d_z             dirs = w / sqrt((w_x^2 + w_y^2) + w_z^2)
 *     c = float(byte) / 255,  a likewise
 *     3 channels     rgb = c, mask = 1
 *     white          rgb = clamp(c * a + (1 - a), 0, 1)        black   rgb = clamp(c - (1 - a), 0, 1)        mask = a > 0.5
 * A ray whose view index is outside [0, num_views) or whose pixel index is outside [0, H W) reads nothing and gets NaN in its
 * rows of origins, dirs and rgb and 0 in mask; every other ray is unaffected. One lane makes one ray; no workspace, no
 * allocation, no synchronisation, no atomics: capturable, and two calls return the same bits. Validation precedes any HIP call:
 * SHACIRA_EINVAL for num_views, width or height <= 0, W * H >= 2^31, n < 0, channels outside {3, 4} with images, an unknown
 * bg_mode, only one of the two index arrays, n > num_views * H * W in the whole-view form, NULL cams / origins / dirs (rgb /
 * mask with images), or a misaligned cams / jitter. n == 0 returns 0 with nothing enqueued, whatever the pointers (the sizes,
 * channels and bg_mode are checked first).
 */
#define SHACIRA_RAYGEN_RECORD_FLOATS 20
#define SHACIRA_RAYGEN_BG_WHITE 0
#define SHACIRA_RAYGEN_BG_BLACK 1
SHACIRA_API int shacira_raygen_record_floats(void);
SHACIRA_API int shacira_raygen(const float *cams, int num_views, int width, int height, const int32_t *view_idx,
                               const int32_t *pixel_idx, const float *jitter, int64_t n, const uint8_t *images, int channels,
                               int bg_mode, float *origins, float *dirs, float *rgb, uint8_t *mask, void *stream);

/*
 * Mip levels of the training images: a power-of-two area resize (OpenCV's INTER_AREA by 2^-mip, what
 * wisp/datasets/formats/nerf_standard_dataset.py:221 asks of cv2) is the mean of a 2^mip x 2^mip block of pixels. Its numerator
 * is an integer that fits 16 bits for mip <= SHACIRA_IMAGE_MIP_MAX (255 * 4^4 = 65280), so a level is kept EXACTLY, as one uint16
 * sum per channel -- 8 bytes per RGBA pixel of the level -- and divided once, where a colour is needed.
 * shacira_image_mip:
 *   images         uint8 [num_views, height, width, channels] on the device, channels 1 .. 4
 *   mip            1 .. SHACIRA_IMAGE_MIP_MAX; height and width are multiples of 2^mip
 *   sums           uint16 [num_views, height >> mip, width >> mip, channels], overwritten:
 *                     sums[v, y, x, c] = sum over dy, dx < 2^mip of images[v, (y << mip) + dy, (x << mip) + dx, c]
 * Every byte offset is 64-bit: num_views * height * width * channels may pass 2^31. One pass over the source bytes, lanes along
 * x; four channels on a 4-byte aligned `images` and 8-byte aligned `sums` read dwords (16 bytes per lane when `images` is 16-byte
 * aligned) and store a pixel's four sums at once, anything else reads bytes -- the result is the same. No workspace, no
 * allocation, no synchronisation, no atomics, no LDS: capturable, two calls return the same bits. Validation precedes any HIP
 * call: SHACIRA_EINVAL for mip outside 1 .. 4, channels outside 1 .. 4, num_views, height or width <= 0, height or width not a
 * multiple of 2^mip, (height >> mip) * (width >> mip) >= 2^31, a byte count beyond 2^60, a NULL pointer or an odd `sums`.
 * shacira_raygen_sums: shacira_raygen with the colours of a mip level. Every argument and every rule above (shacira_raygen) holds
 * with `sums` uint16 [num_views, H, W, channels] (2-byte aligned; W, H are the LEVEL's size) in the place of `images`, and
 *     c = float(S) / float(255 << (2 mip)),  a likewise
 * -- two exactly representable numbers and one correctly rounded division, so c is the correctly rounded block mean -- in the
 * place of float(byte) / 255; the composite, the clamp, the NaN rows and the whole-view form are the same code. mask = a > 0.5
 * is the integer test 2 S_a > 255 * 4^mip: at equality a is exactly 0.5, and one unit of S_a above it a exceeds 0.5 by 1 / (255 *
 * 4^mip) >= 2^-16, far above fp32's spacing there. Four channels on an 8-byte aligned base take one 8-byte load per ray.
 * SHACIRA_EINVAL additionally for mip outside 1 .. SHACIRA_IMAGE_MIP_MAX.
 */
#define SHACIRA_IMAGE_MIP_MAX 4
SHACIRA_API int shacira_image_mip(const uint8_t *images, int64_t num_views, int64_t height, int64_t width, int channels,
                                  int mip, uint16_t *sums, void *stream);
SHACIRA_API int shacira_raygen_sums(const float *cams, int num_views, int width, int height, const int32_t *view_idx,
                                    const int32_t *pixel_idx, const float *jitter, int64_t n, const uint16_t *sums,
                                    int channels, int mip, int bg_mode, float *origins, float *dirs, float *rgb,
                                    uint8_t *mask, void *stream);

/*
 * Structured point clouds (ABI 11, additive): a coloured structured point cloud (SPC) built from depth images or from a point
 * cloud, and its first-hit tracer -- the reference's RGB-D path (wisp/datasets/formats/rtmv_dataset.py, wisp/ops/pointcloud,
 * wisp/models/nefs/spc_field.py, wisp/tracers/packed_spc_tracer.py) from the data that stay on the device: the uint8 images (or
 * a mip level's uint16 sums), one fp32 depth plane and the camera records of shacira_raygen.
 *
 * Device layout of an SPC of level L, 1 <= L <= SHACIRA_OCTREE_MAX_LEVEL, G = 2^L:
 *   words    int32 [shacira_spc_num_words(L) = max(1, G^3 / 32)]: cell (x, y, z) has key (x G + y) G + z and is bit key & 31 of
 *            word key >> 5 -- the layout of OctreeAS.packed_occupancy and shacira_mesh_voxelize; unused bits are 0
 *   rank     int32 [same length]: the number of set bits in all earlier words (an exclusive prefix), so that
 *            slot(key) = rank[key >> 5] + popc(words[key >> 5] & ((1u << (key & 31)) - 1)) numbers the cells in key order
 *   colors   uint8 [cells, 4]: RGBA by slot, A = 255
 *
 * The depth entries share (cams, num_views, width, height) of shacira_raygen (num_views may be 0: nothing to do) and
 *   depth    fp32 [num_views, H, W]. A pixel is VALID iff its depth is finite.
 * The POINT of a valid pixel (v, y, x): shacira_raygen's origin o and unit direction d of that pixel without jitter, then
 *     s_i = d_i * depth (one rounding)     p_i = o_i + s_i (one rounding)     -- no fused multiply-add.
 * The COLOUR of a pixel: shacira_raygen's (mip 0: images uint8) or shacira_raygen_sums' (mip 1 .. 4: images are the uint16 sums,
 * width and height the level's) composited fp32 colour c over bg_mode, quantised q = (uint8) rintf(255 * c).
 * The CELL of a point at level L (OctreeAS.quantize_pointcloud): per axis floorf((x + 1) * 0.5f * G); a point with a cell that is
 * not finite is dropped, every other cell is clamped to 0 .. G - 1 (x = 1 falls into the last cell).
 *
 * shacira_depth_bounds         bounds fp32 [6] = min x, y, z, max x, y, z of the points of all valid pixels, count int64 [1] =
 *                              their number; both are initialised by the call, on the stream. No valid pixel: +inf, -inf, 0. Min
 *                              and max are taken with integer atomics on an order-preserving image of the floats: the result does
 *                              not depend on the order, two calls return the same bits.
 * shacira_depth_points_count   block_counts int32 [ceil(V H W / 256)]: the valid pixels among each 256 consecutive ones
 * shacira_depth_points_emit    the compacted cloud in (view, pixel) order: points fp32 [M, 3] and, when rgb != NULL, the colour
 *                              bytes uint8 [M, 3] (images, channels, mip, bg_mode are then required; ignored otherwise).
 *                              block_offsets int64 [blocks] is the caller's exclusive scan of block_counts. Two calls return the
 *                              same bits.
 * shacira_spc_mark_points      ORs the bit of the cell of every point of points fp32 [n, 3] into `words`, which the caller zeroed
 * shacira_spc_mark_depth       the same for the points of the valid pixels; the cloud is never materialised
 * shacira_spc_rank             rank[w] = popc(words[w]) for every word: the caller's exclusive scan (integers: exact) turns it
 *                              into `rank`, and the inclusive total is the cell count -- on the device, no read-back here
 * shacira_spc_accumulate_points / _depth    adds (q_R, q_G, q_B, 1) into sums uint64 [cells, 4] (zeroed by the caller) at the slot
 *                              of the point's cell, with 64-bit integer atomics: exact, so independent of the order. _points
 *                              takes the bytes rgb uint8 [n, 3]. A point whose cell is not set in `words`, or whose slot is
 *                              outside [0, cells), adds nothing.
 * shacira_spc_resolve          colors[slot, c] = (2 sum_c + n) / (2 n) by integer division (the mean rounded to nearest, ties
 *                              up), A = 255; a slot with n = 0 gets (0, 0, 0, 255)
 * shacira_spc_first_hit        origins, dirs fp32 [num_rays, 3]; colors may be NULL (rank and rgb are then not read / written).
 *                              One lane per ray writes depth fp32 [N], hit uint8 [N], pidx int32 [N] (the Morton index of the
 *                              cell, x most significant, as shacira_raytrace_dense_emit writes it) and rgb fp32 [N, 3] =
 *                              byte / 255. A miss writes 0 / 0 / -1 / (0, 0, 0). A ray with a component of its origin or
 *                              direction that is not finite is a miss, tested before anything else. Every other ray gets the
 *                              FIRST nugget shacira_raytrace_dense_emit writes for it on the same occupied set: the same pidx,
 *                              and its entry depth bit for bit -- the walk is that kernel's arithmetic (slab test, tmax += tdelta,
 *                              tie order x, y, z), only the occupancy is read from the packed words.
 * Validation precedes any HIP call and returns SHACIRA_EINVAL: a negative count, width or height <= 0, W H >= 2^31, more than
 * 2^31 - 1 workgroups of 256 pixels, level outside 1 .. 10, channels outside {3, 4}, mip outside 0 .. 4 or an unknown bg_mode
 * where colours are made, num_rays >= 2^31, a NULL or misaligned operand (cams 16 bytes, sums and count 8, words / rank / colors
 * / floats 4, uint16 images 2). n == 0 (no view, no point, no ray, no cell) returns 0 with nothing enqueued. Every entry runs on
 * `stream`, allocates nothing and never synchronises with the host.
 */
SHACIRA_API size_t shacira_spc_num_words(int level);
SHACIRA_API int shacira_depth_bounds(const float *cams, int num_views, int width, int height, const float *depth, float *bounds,
                                     int64_t *count, void *stream);
SHACIRA_API int shacira_depth_points_count(const float *cams, int num_views, int width, int height, const float *depth,
                                           int32_t *block_counts, void *stream);
SHACIRA_API int shacira_depth_points_emit(const float *cams, int num_views, int width, int height, const float *depth,
                                          const void *images, int channels, int mip, int bg_mode, const int64_t *block_offsets,
                                          float *points, uint8_t *rgb, void *stream);
SHACIRA_API int shacira_spc_mark_points(int64_t n, const float *points, int level, uint32_t *words, void *stream);
SHACIRA_API int shacira_spc_mark_depth(const float *cams, int num_views, int width, int height, const float *depth, int level,
                                       uint32_t *words, void *stream);
SHACIRA_API int shacira_spc_rank(int level, const uint32_t *words, int32_t *rank, void *stream);
SHACIRA_API int shacira_spc_accumulate_points(int64_t n, const float *points, const uint8_t *rgb, int level,
                                              const uint32_t *words, const int32_t *rank, int64_t cells, uint64_t *sums,
                                              void *stream);
SHACIRA_API int shacira_spc_accumulate_depth(const float *cams, int num_views, int width, int height, const float *depth,
                                             const void *images, int channels, int mip, int bg_mode, int level,
                                             const uint32_t *words, const int32_t *rank, int64_t cells, uint64_t *sums,
                                             void *stream);
SHACIRA_API int shacira_spc_resolve(int64_t cells, const uint64_t *sums, uint8_t *colors, void *stream);
SHACIRA_API int shacira_spc_first_hit(int64_t num_rays, const float *origins, const float *dirs, int level,
                                      const uint32_t *words, const int32_t *rank, const uint8_t *colors, float *depth,
                                      uint8_t *hit, int32_t *pidx, float *rgb, void *stream);

/*
 * Pixel batches and the pixel loss: an image fit's coordinates, target colours, squared error and "clamped PSNR" statistics made
 * from pixel indices and ONE uint8 image that stays on the device -- what wisp/datasets/formats/multi_image_dataset.py:140-161
 * stores per pixel (40 bytes on the host) and :190-242 gathers per batch, and what wisp/ops/image/metrics.py:39-58 computes from a
 * materialised fp32 target. Operands common to the three calls:
 *   image          uint8 [height, width, 3], contiguous, on the device; height, width in 1 .. 2^31 - 1. Every byte offset is
 *                  64-bit: an image of 2^31 bytes or more works
 *   pixel_idx      int32 [n] (idx_bits == 32) or int64 [n] (idx_bits == 64), pixel p = y * width + x. NULL: the range form, pixel
 *                  i is start + i, with 0 <= start and start + n <= height * width (start is ignored with indices)
 *   n              rows; 0 returns 0 with nothing enqueued, whatever the pointers (sizes, idx_bits and strides are checked first)
 * shacira_pixel_batch: coords fp32 [n, 2] and rgb fp32 [n, 3], dense; either may be NULL (not written), not both. fp32, one
 * rounding per operator as written (correctly rounded divisions, no fused multiply-add), y = p / width and x = p - y * width in
 * integers:
 *     coords = (((float)y / (float)height - 0.5f) * 2.0f, ((float)x / (float)width - 0.5f) * 2.0f)        the ROW comes first
 *     rgb[c] = (float)byte[c] / 255.0f
 * the reference's lattice (multi_image_dataset.py:148-153) and torchvision's ToTensor. The integer split is exact for every image;
 * the reference's transform_coords (:232-242) divides the index by an fp32 tensor and agrees with it only up to 2^24 pixels. An
 * index outside [0, height * width) reads nothing and gets NaN in its rows; every other row is unaffected. No workspace, no
 * atomics: capturable, two calls return the same bits.
 * shacira_pixel_loss_forward: pred fp32 [n, >= 3] with pred_stride >= 3 floats between rows (only the first three columns are
 * read), stats fp64 [3] on the device, overwritten. Per pixel and channel:
 *     d        = pred - (float)byte / 255.0f               fp32, one rounding each, as torch computes pred - target
 *     stats[0] += (double)d * (double)d                    a NaN or infinite prediction shows here
 *     lvl      = (uint8)(min(max(pred, 0), 1) * 255.0f)    truncated; a NaN prediction gives level 0
 *     stats[1] += (lvl - byte)^2                           integers: this sum is exact (the target's own level IS its byte)
 *   stats[2] = the number of pixels that counted. An index out of range is skipped: its row of pred is not read and it is not
 *   counted. out_image uint8 [height, width, 3] or NULL: the three levels are stored at the pixel's place, every other byte is
 *   left alone. Duplicate indices in one call race on out_image (one of the duplicates' levels is kept); stats does not depend
 *   on it. workspace: shacira_pixel_loss_workspace_bytes(n) bytes (0 for n <= 0): one partial of SHACIRA_PIXEL_PARTIAL_BYTES per
 *   workgroup, at most SHACIRA_PIXEL_MAX_GRID of them. Each workgroup adds its pixels in a fixed order in fp64, a one-workgroup
 *   finish kernel adds the partials in a fixed order: no floating-point atomics, two calls return the same bits.
 * shacira_pixel_loss_backward: grad_pred fp32 [n, 3] dense, overwritten: grad_pred[i, c] = g * (2.0f * d) with g = grad[0] read
 * from the device (no read-back) -- the single rounding per product of torch's backward of ((pred - target) ** 2).sum(), so the
 * same bits. Skipped rows get 0.
 * Validation precedes any HIP call: SHACIRA_EINVAL for height or width outside 1 .. 2^31 - 1, n < 0, idx_bits outside {32, 64}
 * with indices, a range that leaves the image, pred_stride < 3 or n * pred_stride beyond 2^59, a NULL operand (image; coords and
 * rgb both; pred, stats, grad, grad_pred), a missing or short workspace. Everything runs on `stream` without allocation or
 * synchronisation.
 */
#define SHACIRA_PIXEL_MAX_GRID 2048
#define SHACIRA_PIXEL_PARTIAL_BYTES 24
SHACIRA_API int shacira_pixel_batch(const uint8_t *image, int64_t height, int64_t width, const void *pixel_idx, int idx_bits,
                                    int64_t start, int64_t n, float *coords, float *rgb, void *stream);
SHACIRA_API size_t shacira_pixel_loss_workspace_bytes(int64_t n);
SHACIRA_API int shacira_pixel_loss_forward(const float *pred, int64_t pred_stride, const uint8_t *image, int64_t height,
                                           int64_t width, const void *pixel_idx, int idx_bits, int64_t start, int64_t n,
                                           uint8_t *out_image, double *stats, void *workspace, size_t workspace_bytes,
                                           void *stream);
SHACIRA_API int shacira_pixel_loss_backward(const float *pred, int64_t pred_stride, const uint8_t *image, int64_t height,
                                            int64_t width, const void *pixel_idx, int idx_bits, int64_t start, int64_t n,
                                            const float *grad, float *grad_pred, void *stream);

/*
 * Latent decode, deterministic (non-SGA) path of LatentDecoder.forward with num_layers_dec == 0
 * (basic_latent_decoder.py:192-198 with DecoderLayer.forward :86-91):
 *     q        = rint(latent)                       round-half-to-even, torch.round (StraightThrough :28-36)
 *     z[c]     = q[c] / div[c]
 *     y[j]     = (sum_c z[c] * matrix[c, j]) * colscale[j] + shift[j]
 *     decoded  = clamp(y, -clamp_weights, +clamp_weights) if clamp_weights > 0
 *   'sq'  decoders pass matrix = scale [latent_dim, feature_dim], colscale = NULL (treated as 1);
 *   'dft' decoders pass matrix = dft   [latent_dim, feature_dim], colscale = scale [feature_dim].
 *   shift may be NULL (use_shift False). All fp32.
 *
 * Backward (straight-through for the rounding): given grad_decoded [T, feature_dim]
 *     grad_latent[c]   = (sum_j gy[j] * colscale[j] * matrix[c, j]) / div[c]            (gy zeroed where clamped)
 *     grad_matrix[c,j] = sum_T z[c] * gy[j] * colscale[j]          ('sq': this is grad(scale))
 *     grad_colscale[j] = sum_T gy[j] * (sum_c z[c] * matrix[c, j]) ('dft': this is grad(scale))
 *     grad_shift[j]    = sum_T gy[j]
 *   Any of grad_latent / grad_matrix / grad_colscale / grad_shift may be NULL (not computed). Reductions over T
 *   are accumulated in fp64 partials held in `workspace` and written (not accumulated) to the outputs.
 */
SHACIRA_API int shacira_latent_decode_forward(int64_t num_rows, int latent_dim, int feature_dim, const float *latent,
                                  const float *div, const float *matrix, const float *colscale,
                                  const float *shift, float clamp_weights, float *decoded, void *stream);

SHACIRA_API size_t shacira_latent_decode_backward_workspace_bytes(int64_t num_rows, int latent_dim, int feature_dim);

SHACIRA_API int shacira_latent_decode_backward(int64_t num_rows, int latent_dim, int feature_dim, const float *latent,
                                   const float *div, const float *matrix, const float *colscale,
                                   const float *shift, float clamp_weights, const float *grad_decoded,
                                   float *grad_latent, float *grad_matrix, float *grad_colscale,
                                   float *grad_shift, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Entropy bits of the latents under the factorised BitEstimator (latent_grid.py:122-136,
 * bit_estimator.py:27-65):
 *     w     = latent + noise           (noise != NULL: training)   or   rint(latent)   (noise == NULL: is_val)
 *     p     = CDF(w + 0.5) - CDF(w - 0.5)
 *     bits  = clamp(-log(p + 1e-10) / ln 2, 0, 50)
 *     *total_bits = sum over all [num_rows, latent_dim] entries          (fp32 scalar on the device)
 *   CDF: for each of the first (num_layers-1) of {f1,f2,f3}: x = x*softplus(h)+b ; x = x + tanh(x)*tanh(a);
 *        then f4: sigmoid(x*softplus(h)+b).   params = fp32 [4][3][latent_dim] = (f1.h,f1.b,f1.a, f2..., f4.h,f4.b,unused)
 *
 * Backward, given the upstream scalar gradient d(loss)/d(total_bits) (device fp32 scalar):
 *     grad_latent [num_rows, latent_dim]   (zero where noise == NULL: round() has zero gradient; and where clamped)
 *     grad_params fp32 [4][3][latent_dim]  (unused slots written as 0)
 *   Either output may be NULL.
 */
SHACIRA_API size_t shacira_entropy_bits_workspace_bytes(int64_t num_rows, int latent_dim);

SHACIRA_API int shacira_entropy_bits_forward(int64_t num_rows, int latent_dim, int num_layers, const float *latent,
                                 const float *noise, const float *params, float *total_bits, void *workspace,
                                 size_t workspace_bytes, void *stream);

SHACIRA_API int shacira_entropy_bits_backward(int64_t num_rows, int latent_dim, int num_layers, const float *latent,
                                  const float *noise, const float *params, const float *grad_total_bits,
                                  float *grad_latent, float *grad_params, void *workspace, size_t workspace_bytes,
                                  void *stream);

/*
 * Fused decoder MLP (row a14): BasicDecoder.forward of the reference (wisp/models/decoders/basic_decoders.py:74-101)
 * as NeuralImage uses it (wisp/models/nefs/image.py:107-116, :152): `num_hidden` Linear(+bias)+ReLU layers of width
 * `hidden_dim`, then the linear `lout`; fp32.
 *   params / grad_params: one flat buffer  W1 [H, IN] (nn.Linear.weight layout), b1 [H], W2 [H, H], b2 [H], ...,
 *                         Wout [OUT, H], bout [OUT]
 *   x [num_rows, in_dim], y / grad_y [num_rows, out_dim], grad_x [num_rows, in_dim] (may be NULL)
 * Only a fixed set of shapes is compiled (shacira_mlp_supported); others return SHACIRA_EDTYPE and the caller keeps
 * using its own Linear layers. The backward recomputes the hidden activations (nothing is saved by the forward).
 * (Behaviour tightened within ABI 11, no signature change: the alignment refusal below is new -- such pointers were launched
 * on before -- and so is the NaN rule; a caller that passed aligned, finite operands sees the same results to fp32 rounding.)
 * Alignment: rows of 4n floats are moved as 16-byte vectors, so x and grad_x must be 16-byte aligned when in_dim % 4 == 0
 * and y when out_dim % 4 == 0; otherwise SHACIRA_EINVAL and nothing runs. params, grad_y, grad_params need 4 bytes only.
 * Non-finite values: the ReLU is torch.relu's -- a NaN pre-activation gives a NaN activation, and a NaN activation passes
 * its upstream gradient on (only h <= 0 blocks it) -- so a row with a NaN feature has a NaN output row.
 * num_rows == 0: the forward does nothing; the backward writes grad_params = 0 (x, grad_y, grad_x may be NULL).
 */
SHACIRA_API int shacira_mlp_supported(int in_dim, int hidden_dim, int num_hidden, int out_dim);
SHACIRA_API size_t shacira_mlp_backward_workspace_bytes(int in_dim, int hidden_dim, int num_hidden, int out_dim);
SHACIRA_API int shacira_mlp_forward(int64_t num_rows, int in_dim, int hidden_dim, int num_hidden, int out_dim, const float *x,
                        const float *params, float *y, void *stream);
SHACIRA_API int shacira_mlp_backward(int64_t num_rows, int in_dim, int hidden_dim, int num_hidden, int out_dim, const float *x,
                         const float *params, const float *grad_y, float *grad_x, float *grad_params, void *workspace,
                         size_t workspace_bytes, void *stream);

/*
 * Fused Adam step over a flat fp32 buffer ("next" row f1: the optimizer step that follows the backward in the
 * reference's trainers, torch.optim.Adam built by wisp/trainers/base_trainer.py:206-266 and stepped at
 * wisp/trainers/image_trainer.py:355-359). torch.optim.Adam semantics with amsgrad=False, maximize=False:
 *     g' = grad + weight_decay*param ; m = beta1*m + (1-beta1)*g' ; v = beta2*v + (1-beta2)*g'^2
 *     param -= lr/(1-beta1^step) * m / (sqrt(v)/sqrt(1-beta2^step) + eps)
 *   step counts from 1. zero_grad != 0 also clears `grad` in the same pass (saves the next step's memset).
 */
SHACIRA_API int shacira_adam_step(int64_t numel, float *param, float *grad, float *exp_avg, float *exp_avg_sq, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int step, int zero_grad, void *stream);

/* Same, with the step count read from DEVICE memory (int32, >= 1) so that the launch can be captured into a
 * hipGraph and replayed while the count advances (the caller increments it on the stream). */
SHACIRA_API int shacira_adam_step_capturable(int64_t numel, float *param, float *grad, float *exp_avg, float *exp_avg_sq,
                                 float lr, float beta1, float beta2, float eps, float weight_decay,
                                 const int32_t *step_dev, int zero_grad, void *stream);

/* Multi-tensor form: up to 32 parameters (HOST arrays of device pointers, sizes, per-tensor lr / weight decay) in
 * one launch. `step_dev` non-NULL: step count read from device memory (graph-capturable), else `step` is used. */
SHACIRA_API int shacira_adam_step_multi(int num_tensors, const int64_t *numel_host, float *const *param, float *const *grad,
                            float *const *exp_avg, float *const *exp_avg_sq, const float *lr_host,
                            const float *weight_decay_host, float beta1, float beta2, float eps, int step,
                            const int32_t *step_dev, int zero_grad, void *stream);

/*
 * Loss-scaled steps for mixed-precision training (the reference trains under autocast + torch.cuda.amp.GradScaler,
 * wisp/trainers/base_trainer.py:167-168) with no host round trip. Two more DEVICE pointers, either may be NULL:
 *   found_inf_dev   one float. Every workgroup reads it first; non-zero SKIPS the step: param and all state stay bit
 *                   for bit as they were, and so does grad unless zero_grad != 0, which still clears it (a persistent
 *                   gradient buffer must not carry an inf into the next accumulation). NULL: never skip.
 *   grad_scale_dev  one float, the loss scale. The gradient is unscaled first, gu = grad / *grad_scale_dev, rounded to
 *                   fp32 on its own (never fused into the weight-decay product: a power-of-two scale changes no bit of
 *                   the step). With zero_grad == 0, gu is written back to grad (as torch's fused optimizers do);
 *                   otherwise grad is cleared. NULL: the gradients are already unscaled, grad is not rewritten.
 *                   With a scale that is no power of two the division's remainder (grad - gu*scale, exact) is carried
 *                   into the state beside gu, so the moments follow grad / scale more closely than fp32 gu alone would.
 * A skipped step must not advance a device-resident step count: the caller adds (found_inf == 0) to it on the stream.
 * With both pointers NULL shacira_adam_step_multi_scaled IS shacira_adam_step_multi.
 */
SHACIRA_API int shacira_adam_step_multi_scaled(int num_tensors, const int64_t *numel_host, float *const *param,
                            float *const *grad, float *const *exp_avg, float *const *exp_avg_sq, const float *lr_host,
                            const float *weight_decay_host, float beta1, float beta2, float eps, int step,
                            const int32_t *step_dev, int zero_grad, const float *grad_scale_dev,
                            const float *found_inf_dev, void *stream);

/*
 * Multi-tensor RMSprop (nerf_base.yaml's optimizer_type 'rmsprop'): torch.optim.RMSprop with centered=False,
 * maximize=False, up to 32 parameters in one launch, table layout as shacira_adam_step_multi:
 *     g' = grad + weight_decay*param ; sq = alpha*sq + (1-alpha)*g'^2 ; avg = sqrt(sq) + eps
 *     momentum == 0: param -= lr * g'/avg          otherwise: buf = momentum*buf + g'/avg ; param -= lr*buf
 *   momentum_buf may be NULL when momentum == 0 (it is not read). grad_scale_dev / found_inf_dev / zero_grad as above.
 */
SHACIRA_API int shacira_rmsprop_step_multi(int num_tensors, const int64_t *numel_host, float *const *param,
                            float *const *grad, float *const *square_avg, float *const *momentum_buf,
                            const float *lr_host, const float *weight_decay_host, float alpha, float eps,
                            float momentum, const float *grad_scale_dev, const float *found_inf_dev, int zero_grad,
                            void *stream);

/*
 * Latent decode with stochastic Gumbel annealing (SGA) instead of rounding -- the `use_sga` branch of
 * LatentDecoder.forward (wisp/models/latent_decoders/basic_latent_decoder.py:183-191), the training mode of the
 * reference's shipped configs (kodak.yaml / nerf_lego.yaml: use_sga, diff_sampling) until `decay_period`:
 *     wf = floor(w), wc = wf + 1
 *     logits = -tanh(clamp(w - wf, +-(1 - 1e-6))) / T ,  -tanh(clamp(wc - w, +-(1 - 1e-6))) / T
 *     (s0, s1) = RelaxedOneHotCategorical(T, logits).rsample()      [diff_sampling]  /  .sample()  [otherwise]
 *              = softmax((logits + g) / T),  g = -log(-log(clamp(u, eps, 1 - eps)))
 *     q = wf * s0 + wc * s1 ;  then the decode of shacira_latent_decode_forward on q instead of round(w).
 * `uniforms` [num_rows, latent_dim, 2] fp32 in [0, 1) are supplied by the caller (torch.rand on the device: the one
 * draw the reference's sampler makes), so the operator is deterministic. Backward: grad_latent through rsample() when
 * diff_sampling (floor carries no gradient), through a straight-through floor otherwise; other outputs as in
 * shacira_latent_decode_backward.
 */
SHACIRA_API int shacira_latent_decode_sga_forward(int64_t num_rows, int latent_dim, int feature_dim, const float *latent,
                                      const float *uniforms, float temperature, int diff_sampling, const float *div,
                                      const float *matrix, const float *colscale, const float *shift,
                                      float clamp_weights, float *decoded, void *stream);
SHACIRA_API int shacira_latent_decode_sga_backward(int64_t num_rows, int latent_dim, int feature_dim, const float *latent,
                                       const float *uniforms, float temperature, int diff_sampling, const float *div,
                                       const float *matrix, const float *colscale, const float *shift,
                                       float clamp_weights, const float *grad_decoded, float *grad_latent,
                                       float *grad_matrix, float *grad_colscale, float *grad_shift, void *workspace,
                                       size_t workspace_bytes, void *stream);
/* ABI 9: the same pair with the temperature in DEVICE memory (one float the kernels read): a training step captured into a
 * HIP graph anneals it between replays (base_trainer.py:155-157 decays it every iteration) without re-capturing. */
SHACIRA_API int shacira_latent_decode_sga_forward_tdev(int64_t num_rows, int latent_dim, int feature_dim,
                                       const float *latent, const float *uniforms, const float *temperature_dev,
                                       int diff_sampling, const float *div, const float *matrix, const float *colscale,
                                       const float *shift, float clamp_weights, float *decoded, void *stream);
SHACIRA_API int shacira_latent_decode_sga_backward_tdev(int64_t num_rows, int latent_dim, int feature_dim,
                                       const float *latent, const float *uniforms, const float *temperature_dev,
                                       int diff_sampling, const float *div, const float *matrix, const float *colscale,
                                       const float *shift, float clamp_weights, const float *grad_decoded,
                                       float *grad_latent, float *grad_matrix, float *grad_colscale, float *grad_shift,
                                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * Latent decoder WITH hidden layers / activations -- LatentDecoder with num_layers_dec > 0 and / or activation,
 * final_activation != 'none' (wisp/models/latent_decoders/basic_latent_decoder.py:97-198: the layer stack :139-147, forward
 * :182-198, DecoderLayer.forward :86-91, SineScaled(30.0) wisp/models/activations): a per-row MLP over the table,
 *     decoded = clamp(final_act(L_n(act(... act(L_1(q(latent) / div)) ...)))),     L_k(x) = x @ W_k + b_k,
 * q = round (straight-through) or, with uniforms != NULL, the SGA sample of the operators above. One pass each way.
 *   num_layers   hidden layers + 1, 1 .. SHACIRA_LATENT_MLP_MAX_LAYERS
 *   widths_host  HOST int32 [num_layers + 1]: latent_dim, hidden widths ..., feature_dim; each 1 .. SHACIRA_LATENT_MLP_MAX_WIDTH
 *   params       device fp32, packed per layer: W_k [widths[k], widths[k+1]] row-major (the layer's effective matrix: `scale`
 *                for 'sq', `dft * scale` for 'dft*'), then b_k [widths[k+1]] (`shift`; zeros when the layer has none)
 *   activation / final_activation   SHACIRA_ACT_* (the reference's act_dict keys)
 *   backward: grad_latent [num_rows, latent_dim] (NULL = skip), grad_params packed like params (the caller chains it to
 *   scale / shift); workspace of shacira_latent_mlp_backward_workspace_bytes() bytes (fp64 block partials: the table
 *   reductions are bitwise reproducible).
 * Returns SHACIRA_EINVAL for shapes outside the limits (the caller keeps its own per-layer evaluation for those).
 */
#define SHACIRA_LATENT_MLP_MAX_LAYERS 4
#define SHACIRA_LATENT_MLP_MAX_WIDTH 16
#define SHACIRA_ACT_NONE 0
#define SHACIRA_ACT_SIGMOID 1
#define SHACIRA_ACT_TANH 2
#define SHACIRA_ACT_RELU 3
#define SHACIRA_ACT_SINE30 4
SHACIRA_API int shacira_latent_mlp_supported(int num_layers, const int32_t *widths_host);
SHACIRA_API size_t shacira_latent_mlp_backward_workspace_bytes(int num_layers, const int32_t *widths_host);
SHACIRA_API int shacira_latent_mlp_forward(int64_t num_rows, int num_layers, const int32_t *widths_host, const float *latent,
                               const float *uniforms, float temperature, int diff_sampling, const float *div,
                               const float *params, int activation, int final_activation, float clamp_weights,
                               float *decoded, void *stream);
SHACIRA_API int shacira_latent_mlp_backward(int64_t num_rows, int num_layers, const int32_t *widths_host, const float *latent,
                                const float *uniforms, float temperature, int diff_sampling, const float *div,
                                const float *params, int activation, int final_activation, float clamp_weights,
                                const float *grad_decoded, float *grad_latent, float *grad_params, void *workspace,
                                size_t workspace_bytes, void *stream);

/*
 * Per-level latent decoders -- HierarchicalLatentDecoder (wisp/models/latent_decoders/hierarchical_latent_decoder.py:3-36,
 * built by LatentGrid.setup_decoders, wisp/models/grids/latent_grid.py:176-190): level l decodes the rows
 * [row_offsets[l], row_offsets[l+1]) of the table with ITS OWN div / matrix / colscale / shift; rounding or SGA
 * (uniforms != NULL) as in the single-decoder operators above. One launch for all levels.
 *   row_offsets_host  HOST int64 [num_levels + 1]; level starts ascend. The reference builds the last entry as the LAST
 *                     LEVEL'S SIZE, not the table's end (latent_grid.py:182): a boundary that falls before a level's
 *                     start makes that level empty. Rows no level owns decode to 0 (the reference leaves them
 *                     uninitialised) and receive a zero latent gradient.
 *   div [num_levels, latent_dim], matrix [num_levels, latent_dim, feature_dim], colscale / shift [num_levels,
 *   feature_dim] (NULL as above); the gradients of the backward have the same stacked shapes, written per level.
 */
SHACIRA_API int shacira_latent_decode_levels_forward(int num_levels, const int64_t *row_offsets_host, int64_t num_rows,
                                         int latent_dim, int feature_dim, const float *latent, const float *uniforms,
                                         float temperature, int diff_sampling, const float *div, const float *matrix,
                                         const float *colscale, const float *shift, float clamp_weights,
                                         float *decoded, void *stream);
SHACIRA_API int shacira_latent_decode_levels_backward(int num_levels, const int64_t *row_offsets_host, int64_t num_rows,
                                          int latent_dim, int feature_dim, const float *latent, const float *uniforms,
                                          float temperature, int diff_sampling, const float *div, const float *matrix,
                                          const float *colscale, const float *shift, float clamp_weights,
                                          const float *grad_decoded, float *grad_latent, float *grad_matrix,
                                          float *grad_colscale, float *grad_shift, void *workspace,
                                          size_t workspace_bytes, void *stream);

/*
 * MultiLatentDecoder (wisp/models/latent_decoders/multi_latent_decoder.py:27-210, built by LatentGrid.setup_decoders for
 * `ldecode_type: multi`), no hidden layers: num_decoders affine decoders mixed per table entry by the selector alpha:
 *     a_soft = softmax_k(alpha[k, r] / temperature) ;  a = one-hot(arg-max) if straight_through (gradient: identity) else a_soft
 *     x      = rint(latent[r]) / div            (uniforms == NULL)   or the SGA sample with the same temperature
 *     'dft' (dft != NULL): per_k = (x @ dft) * scale[k, 0, :] + shift[k, :] ;  decoded = sum_k per_k * a_k
 *     'sq'  (dft == NULL): mixed = sum_k (x @ scale[k]) * a_k ;  decoded = sum_k (mixed + shift[k, :]) * a_k
 *       (the reference's forward mixes twice, multi_latent_decoder.py:74-81; kept)
 *   alpha [num_decoders, num_rows]; scale [num_decoders, S, feature_dim] with S = latent_dim ('sq') or 1 ('dft');
 *   dft [latent_dim, feature_dim]; shift [num_decoders, feature_dim] or NULL; clamp as above.
 * Backward writes grad_latent [num_rows, latent_dim] (straight-through rounding / SGA), grad_alpha [num_decoders, num_rows]
 * (through the softmax), grad_scale, grad_shift (NULL = skip, except grad_scale). num_decoders <= 8 and the
 * (latent_dim, feature_dim) pairs of shacira_latent_multi_supported; else SHACIRA_EDTYPE.
 */
SHACIRA_API int shacira_latent_multi_supported(int latent_dim, int feature_dim, int num_decoders);
SHACIRA_API int shacira_latent_multi_decode_forward(int64_t num_rows, int latent_dim, int feature_dim, int num_decoders,
                                        const float *latent, const float *alpha, const float *uniforms,
                                        float temperature, int straight_through, int diff_sampling, const float *div,
                                        const float *scale, const float *dft, const float *shift, float clamp_weights,
                                        float *decoded, void *stream);
SHACIRA_API int shacira_latent_multi_decode_backward(int64_t num_rows, int latent_dim, int feature_dim, int num_decoders,
                                         const float *latent, const float *alpha, const float *uniforms,
                                         float temperature, int straight_through, int diff_sampling, const float *div,
                                         const float *scale, const float *dft, const float *shift, float clamp_weights,
                                         const float *grad_decoded, float *grad_latent, float *grad_alpha,
                                         float *grad_scale, float *grad_shift, void *workspace, size_t workspace_bytes,
                                         void *stream);

/*
 * Symbol statistics and entropy coding of the rounded latents -- replaces the per-channel
 * `torch.round(...).long()` + `torch.unique(return_counts=True)` of LatentGrid.size
 * (wisp/models/grids/latent_grid.py:141-143) and the torchac.encode_float_cdf call (:155-172).
 *
 *   shacira_latent_symbol_range      minmax[c] = {min, max} over rows of (int)rint(latent[r, c])   (device int32 [ld][2];
 *                                    {INT32_MAX, INT32_MIN} when num_rows == 0). rint = round-half-even = torch.round.
 *   shacira_latent_symbol_histogram  counts[c][k] = #rows with rint(latent[r, c]) == minmax[c][0] + k, 0 <= k < nbins
 *                                    (device uint64 [ld][nbins], overwritten). `minmax` is the device array written by
 *                                    shacira_latent_symbol_range; nbins >= max_c (max - min + 1).
 *   latent_dim <= 16, else SHACIRA_EDTYPE.
 *
 * Range coder (HOST buffers, runs on the calling thread; the reference codes on the CPU as well):
 *   static model = freq_host[num_symbols] with sum exactly 65536 and freq >= 1 for every symbol that occurs.
 *   shacira_rc_encode  symbols (indices into the model) -> bytes; *out_len = bytes produced; SHACIRA_EWORKSPACE if
 *                      `capacity` < *out_len (nothing valid written); shacira_rc_encode_bound(n) is always enough.
 *   shacira_rc_decode  exact inverse: reproduces the n symbols.
 */
SHACIRA_API int shacira_latent_symbol_range(int64_t num_rows, int latent_dim, const float *latent, int32_t *minmax,
                                void *stream);
SHACIRA_API int shacira_latent_symbol_histogram(int64_t num_rows, int latent_dim, const float *latent, const int32_t *minmax,
                                    int nbins, uint64_t *counts, void *stream);
SHACIRA_API size_t shacira_rc_encode_bound(int64_t num_symbols_to_code);
SHACIRA_API int shacira_rc_encode(const int32_t *symbols_host, int64_t n, const uint32_t *freq_host, int num_symbols,
                      uint8_t *out_host, size_t capacity, size_t *out_len);
SHACIRA_API int shacira_rc_decode(const uint8_t *in_host, size_t len, const uint32_t *freq_host, int num_symbols, int64_t n,
                      int32_t *symbols_host);

/*
 * Interleaved rANS ("rans64"): the entropy codec that also runs on the device. 64 coder states advance in lockstep and
 * share one stream of 16-bit words, so a 64-lane wavefront codes one block. Integer-exact: the host coder and the kernels
 * produce the same bytes. Added within ABI 11 (new symbols only).
 *
 * Format of ONE channel. Inputs: T symbols s[i] in [0, nbins), nbins >= 2; the model freq[nbins] with sum 65536 and
 * 1 <= freq <= 65535 for every symbol present (shacira_amd/codec.py, normalise_frequencies); cdf[k] = sum(freq[:k]);
 * K = steps per block. A block is 64*K consecutive symbols, nblocks = ceil(T / (64*K)). The state is a 32-bit x in
 * [2^16, 2^32), renormalised in 16-bit words. Lane l at step k of block b owns symbol i = b*64*K + k*64 + l and is active
 * iff i < T; inactive lanes do nothing.
 *
 *   encode block b:  x[0..63] = 0x10000 ; words = []
 *     for k = K-1 down to 0:
 *       for each active lane l (s = its symbol, f = freq[s], c = cdf[s]):  emit[l] = x[l] >= (f << 16)
 *       for lanes with emit, in INCREASING lane order:                     words.append(x[l] & 0xFFFF) ; x[l] >>= 16
 *       for each active lane:                                              x[l] = ((x[l] / f) << 16) + (x[l] % f) + c
 *     output: the 64 final states (u32, lane order) and words (u16), n_b = len(words)
 *
 *   decode block b:  x = states ; p = n_b
 *     for k = 0 .. K-1:
 *       for each active lane:  slot = x & 0xFFFF ; s = the k with cdf[k] <= slot < cdf[k+1]
 *                              x = freq[s] * (x >> 16) + slot - cdf[s]
 *       need[l] = active and x[l] < 0x10000 ; n = count(need) ; r[l] = rank of l among the needing lanes
 *       x[l] = (x[l] << 16) | words[p - n + r[l]]  for needing lanes ; p -= n
 *     on valid input p == 0 and every x == 0x10000 at the end
 *
 * Channel payload, little endian: n_b as u32 x nblocks | final states as u32 x 64 x nblocks, block-major | the words of
 * block 0, block 1, ... as u16. The flush (count + states) is 260 bytes per block: 0.008 bit per symbol at K = 4096.
 * A channel with nbins == 1 carries no payload (its freq would be 65536 and f << 16 would overflow); the decoder fills
 * it with `lo`.
 *
 * Container (shacira_amd/codec.py writes and parses it): magic "SHCR\x02\x00" | u32 header length | JSON header
 * {"coder":"rans64","rows":T,"latent_dim":ld,"steps":K,"channels":[{"lo","nbins","words"}...]} | zero padding to a
 * multiple of 4 | per channel: the frequency table as u16 x nbins (65536 stored as 0), then the channel payload, each
 * zero-padded to a multiple of 4.
 *
 * Host coder (HOST buffers, calling thread), 1 <= steps <= 65536:
 *   shacira_rans_encode_bound  bytes that always hold the payload of n symbols (260 per block + 2 per symbol); 0 for bad steps
 *   shacira_rans_encode        symbols -> channel payload; *out_len = bytes produced; SHACIRA_EWORKSPACE if `capacity` is
 *                              below that. SHACIRA_EINVAL: model sum != 65536, a freq of 65536 (single-symbol channel),
 *                              a symbol outside the model or with freq 0, bad steps, NULL.
 *   shacira_rans_decode        exact inverse. Never reads outside in_host[0, len) or writes outside symbols_host[0, n),
 *                              whatever the bytes: SHACIRA_EINVAL when len != 260*nblocks + 2*sum(n_b), a state is below
 *                              2^16, a block needs more words than it holds (p < 0), or p != 0 / x != 0x10000 at the end.
 *
 * Device coder (one wavefront per (block, channel); everything on `stream`, no synchronisation, no allocation). lo_host,
 * nbins_host, payload_offset_host, words_host are HOST arrays of latent_dim entries, copied into the kernel arguments;
 * `cdf` is a device uint32 [latent_dim][cdf_stride] with cdf[c][0..nbins[c]]; channels with nbins < 2 are skipped.
 * nblocks = ceil(num_rows / (64*steps)); latent_dim <= 16, else SHACIRA_EDTYPE. All validation precedes any HIP call;
 * num_rows == 0 returns 0 and launches nothing.
 *   shacira_latent_rans_encode  reads the fp32 [num_rows, latent_dim] latents, codes symbol (int)rint(v) - lo[c] (clamped
 *                               into the model). Writes counts u32 [ld][nblocks], states u32 [ld][nblocks][64] and each
 *                               block's words into its bound-sized slot, slots u16 [ld][nblocks][64*steps].
 *   shacira_latent_rans_pack    moves counts, states and words to their place in the channel payloads: `out` + the
 *                               channel's payload_offset (bytes, multiple of 4); block_start device int64 [ld][nblocks] =
 *                               exclusive prefix of the channel's counts; words_host[c] = their sum. SHACIRA_EINVAL when a
 *                               payload would end beyond out_bytes. Starts and counts are clamped into the channel's words.
 *   shacira_latent_rans_decode  `container` = the container's bytes on the device (4-byte aligned); writes
 *                               symbol + lo[c] as fp32 into out [num_rows, latent_dim]. cdf is searched from LDS when
 *                               max nbins < 4096, from global memory otherwise. Every word index is clamped into its
 *                               block's [0, n_b), the block into the channel's words, the symbol into [0, nbins): corrupt
 *                               bytes give wrong values, never an access outside the container. *error (device int32,
 *                               zeroed by the caller) is set to 1 on an underflow, a state below 2^16 or a bad end state.
 *                               SHACIRA_EINVAL when a payload would end beyond container_bytes.
 */
SHACIRA_API size_t shacira_rans_encode_bound(int64_t num_symbols_to_code, int steps);
SHACIRA_API int shacira_rans_encode(const int32_t *symbols_host, int64_t n, const uint32_t *freq_host, int num_symbols,
                        int steps, uint8_t *out_host, size_t capacity, size_t *out_len);
SHACIRA_API int shacira_rans_decode(const uint8_t *in_host, size_t len, const uint32_t *freq_host, int num_symbols,
                        int64_t n, int steps, int32_t *symbols_host);
SHACIRA_API int shacira_latent_rans_encode(int64_t num_rows, int latent_dim, const float *latent, const int32_t *lo_host,
                               const int32_t *nbins_host, const uint32_t *cdf, int cdf_stride, int steps,
                               uint32_t *counts, uint32_t *states, uint16_t *slots, void *stream);
SHACIRA_API int shacira_latent_rans_pack(int64_t num_rows, int latent_dim, const int32_t *nbins_host, int steps,
                             const uint32_t *counts, const uint32_t *states, const uint16_t *slots,
                             const int64_t *block_start, const int64_t *payload_offset_host, const int64_t *words_host,
                             uint8_t *out, size_t out_bytes, void *stream);
SHACIRA_API int shacira_latent_rans_decode(int64_t num_rows, int latent_dim, const uint8_t *container,
                               size_t container_bytes, const int32_t *lo_host, const int32_t *nbins_host,
                               const int64_t *payload_offset_host, const int64_t *words_host, const uint32_t *cdf,
                               int cdf_stride, const int64_t *block_start, int steps, float *out, int32_t *error,
                               void *stream);

/*
 * Volume integration over variable-length sample packs and sample generation on a dense occupancy grid -- the steps
 * either side of the hash-grid lookup in the NeRF pipeline. The reference runs them through kaolin 0.13 (un-vendored):
 * `spc_render.exponential_integration` / `sum_reduce` (call sites wisp/tracers/packed_rf_tracer.py:131-151),
 * `OctreeAS._raymarch_ray` / `_raymarch_voxel` (wisp/accelstructs/octree_as.py:171-290) on `unbatched_query` /
 * `unbatched_raytrace`.
 *
 * Packs: the samples of ray r are rows [pack_start[r], pack_start[r+1]) (device int64 [num_packs + 1], ascending).
 *   shacira_pack_integrate_forward   weights[i] = exp(-sum_{j<i in pack} tau[j]) * (1 - exp(-tau[i]))
 *                                    ray_feats[r, c] = sum_i weights[i] * feats[i, c]
 *                                    (= exponential_integration(feats, tau, boundary, exclusive=True))
 *   shacira_pack_integrate_backward  gradients of both outputs w.r.t. feats and tau; grad_weights may be NULL (zero)
 *   shacira_pack_sum                 out[r, c] = sum_i x[i, c]                  (= sum_reduce)
 *   shacira_pack_broadcast           out[i, c] = per_pack[r(i), c]              (its gradient)
 *   channels <= 16, else SHACIRA_EDTYPE.
 *
 * Occupancy: uint8 [G][G][G], G = 2^level, indexed [x][y][z]; a point p in [-1,1]^3 lies in cell
 * floor(clamp(G*(p+1)/2, 0, G-1)) (kaolin quantize_points). Both generators are two-pass (count, host/device scan of
 * the counts by the caller, emit at offsets [num_rays + 1]).
 *   shacira_raymarch_ray_{count,emit}    `num_samples` stratified depths per ray:
 *                                        depth = (lin[j] + jitter[r, j] / num_samples) * (dist_max - dist_min) + dist_min
 *                                        (lin = torch.linspace(0, 1, num_samples), jitter ~ U[0,1) supplied by the caller),
 *                                        kept when the cell of origin + dir * depth is occupied. emit writes, in order,
 *                                        ridx int64, samples [.,3], depth, deltas (depth - previous depth of the ray,
 *                                        dist_min before the first), boundary uint8 (1 at a ray's first kept sample).
 *   shacira_raytrace_dense_{count,emit}  every (ray, occupied cell) crossing in depth order: ridx int32, pidx int32
 *                                        (Morton index of the cell, x most significant), depth [., 2] = entry (>= 0), exit.
 */
SHACIRA_API int shacira_pack_integrate_forward(int64_t num_samples, int64_t num_packs, int channels, const float *feats,
                                   const float *tau, const int64_t *pack_start, float *ray_feats, float *weights,
                                   void *stream);
SHACIRA_API int shacira_pack_integrate_backward(int64_t num_samples, int64_t num_packs, int channels, const float *feats,
                                    const float *tau, const int64_t *pack_start, const float *grad_ray_feats,
                                    const float *grad_weights, float *grad_feats, float *grad_tau, void *stream);
SHACIRA_API int shacira_pack_sum(int64_t num_samples, int64_t num_packs, int channels, const float *x,
                     const int64_t *pack_start, float *out, void *stream);
SHACIRA_API int shacira_pack_broadcast(int64_t num_samples, int64_t num_packs, int channels, const float *per_pack,
                           const int64_t *pack_start, float *out, void *stream);
SHACIRA_API int shacira_raymarch_ray_count(int64_t num_rays, int num_samples, const float *origins, const float *dirs,
                               float dist_min, float dist_max, const float *lin, const float *jitter,
                               const uint8_t *occupancy, int level, int32_t *counts, void *stream);
SHACIRA_API int shacira_raymarch_ray_emit(int64_t num_rays, int num_samples, const float *origins, const float *dirs,
                              float dist_min, float dist_max, const float *lin, const float *jitter,
                              const uint8_t *occupancy, int level, const int64_t *offsets, int64_t *ridx,
                              float *samples, float *depth, float *deltas, uint8_t *boundary, void *stream);
/* ABI 9: the same into caller buffers of `capacity` rows -- survivors whose row would be >= capacity are dropped (the
 * caller clamps `offsets` to capacity for its pack reductions). For steps captured into a HIP graph: the buffers cannot
 * be sized from a count read back to the host there. Rows behind the last survivor are left untouched. */
SHACIRA_API int shacira_raymarch_ray_emit_capped(int64_t num_rays, int num_samples, const float *origins,
                              const float *dirs, float dist_min, float dist_max, const float *lin, const float *jitter,
                              const uint8_t *occupancy, int level, const int64_t *offsets, int64_t capacity,
                              int64_t *ridx, float *samples, float *depth, float *deltas, uint8_t *boundary,
                              void *stream);
SHACIRA_API int shacira_raytrace_dense_count(int64_t num_rays, const float *origins, const float *dirs,
                                 const uint8_t *occupancy, int level, int32_t *counts, void *stream);
SHACIRA_API int shacira_raytrace_dense_emit(int64_t num_rays, const float *origins, const float *dirs,
                                const uint8_t *occupancy, int level, const int64_t *offsets, int32_t *ridx,
                                int32_t *pidx, float *depth, void *stream);
/*
 * The 'voxel' marcher (ABI 11, additive): `num_samples` jittered samples inside every occupied crossing, the jitter restated
 * from a seed. Counting is shacira_raytrace_dense_count; the caller scans the counts into `offsets` int64 [num_rays + 1] (in
 * NUGGETS); a ray with c crossings owns the c * num_samples rows from offsets[r] * num_samples on.
 *   nuggets   nugget i of ray r is the i-th crossing shacira_raytrace_dense_emit writes for that ray on the same occupancy,
 *             (t0, t1) bit for bit (the one walk of grid_walk.h).
 *   rows      ordered by ray, nugget, j < num_samples. With u the jitter below and every operator rounded to fp32 on its
 *             own (no fma; 1.0f / num_samples is the fp32 value of the double quotient):
 *               depth    = t0 + (t1 - t0) * ((float(j) + u) * (1.0f / num_samples))
 *               deltas   = depth - depth of row j - 1 of the SAME nugget, t0 before the first (it restarts at every nugget)
 *               samples  = fmaf(dir, depth, origin) per axis
 *               ridx     = r (int64); boundary (uint8) = 1 on row j == 0 of the ray's first nugget, else 0
 *   jitter    u = (w >> 8) * 2^-24 in [0, 1), w = word (j & 3) of Philox4x32-10 with
 *               counter = (c0, c1, c2, c3) = (r, i, j >> 2, low 32 bits of (step + *step_dev))
 *               key     = (k0, k1)         = (low, high 32 bits of seed)
 *             so a sample's jitter depends on (seed, step, r, i, j) only: not on its row, on the capacity or on the other
 *             rays. `step_dev` (device int64, may be NULL = 0) is read when the kernel runs: a captured graph that
 *             increments it draws fresh jitter on every replay. num_rays >= 2^32 is SHACIRA_EINVAL.
 *   capacity  rows of the output buffers; rows >= capacity are dropped, even in the middle of a nugget, the rows behind the
 *             last survivor are left untouched and the caller clamps its row offsets (the contract of
 *             shacira_raymarch_ray_emit_capped). The uncapped call passes capacity = offsets[num_rays] * num_samples.
 *   workspace shacira_raymarch_voxel_workspace_bytes(capacity, num_samples) bytes (the compact nuggets: a thread per ray
 *             walks and writes them, a thread per row expands them), else SHACIRA_EWORKSPACE.
 * num_rays == 0 or capacity == 0 launches nothing and returns 0. num_samples in 1 .. 2^24.
 */
SHACIRA_API size_t shacira_raymarch_voxel_workspace_bytes(int64_t capacity, int num_samples);
SHACIRA_API int shacira_raymarch_voxel_emit(int64_t num_rays, int num_samples, const float *origins, const float *dirs,
                                const uint8_t *occupancy, int level, const int64_t *offsets, uint64_t seed, int64_t step,
                                const int64_t *step_dev, int64_t capacity, void *workspace, size_t workspace_bytes,
                                int64_t *ridx, float *samples, float *depth, float *deltas, uint8_t *boundary,
                                void *stream);

/*
 * Sphere tracing over ray packs (ABI 11, additive): the reference's `find_depth_bound_cuda`
 * (wisp/csrc/render/find_depth_bound_cuda.cu) and, as ONE launch per iteration, the body of the loop of its
 * PackedSDFTracer.trace (wisp/tracers/packed_sdf_tracer.py), which runs there as about 25 masked element-wise launches, a
 * boolean-index compaction and two mask.any() read-backs per iteration.
 *
 * Notation. The nuggets (ray, cell) of a trace are depth [K, 2] fp32 = (entry, exit), sorted by ray and then by depth, as
 * shacira_raytrace_dense_emit writes them. A PACK is the nuggets of one ray: pack p is [first[p], end[p]) with
 * end[p] = first[p + 1], and THE LAST PACK ENDS AT K. Callers pass end[] as pack_end int32 [P]. Indices are int32.
 *
 * find_depth_bound. For pack p with current nugget c = curr_idxes[p] and query depth q = query[p], out[p] is
 *   -1                                   if c < 0;
 *   the first i in [c, end[p]) with (q >= entry_i && q <= exit_i) || q < entry_i;
 *   -1                                   if there is none. A NaN q satisfies neither comparison and gives -1.
 * Every out[p] is written. This is the reference's rule with two of its defects removed:
 *   (a) the reference bounds the walk of pack p by curr_idxes_in[p + 1], the neighbour's CURRENT nugget: once the neighbour
 *       has advanced, the walk of p runs into the neighbour's nuggets. Here the bound is the pack's own end;
 *   (b) for the last pack the reference bounds the walk by num_packs where num_nugs is meant, so the last ray can never
 *       advance (its walk is empty whenever its current nugget is >= num_packs). Here the last pack ends at K.
 * Where the reference stays inside its own pack the two rules agree: every pack but the last on the first call, when
 * curr_idxes is the list of pack starts. (The reference also leaves out[p] unwritten where it finds nothing; its caller
 * pre-fills -1.) The walk never reads past K: pack_end values above num_nugs are treated as num_nugs.
 *
 * Sphere-trace step. Per pack, fp32, one rounding per operator (no contraction: -ffp-contract=off, as for shacira_mesh_sdf).
 * State, structure of arrays over the P packs: t, dist, dist_prev fp32 [P], curr int32 [P], x fp32 [P, 3], active and hit
 * uint8 [P]; o = origins[p], d = dirs[p] are the pack's ray (fp32 [P, 3], gathered per pack by the caller).
 *   Init (the caller's, once per trace):  curr = first[p];  t = entry[curr] (the caller has added 1e-5f to every entry
 *     beforehand, as the reference does in place);  x = o + d * t;  active = 1;  hit = 0.
 *   Iteration i = 0 .. num_steps - 1, for the ACTIVE packs only, given s = sdf(x) evaluated by the caller:
 *     dist = s * step_size;  at i == 0 (first_iteration != 0) also dist_prev = dist
 *     t = t + dist;  x = o + d * t                                  (component-wise: x_k = o_k + d_k * t)
 *     hit = |dist| < min_dis  ||  |dist + dist_prev| * 0.5f < 5.0f * min_dis      (5.0f * min_dis rounded to fp32 once)
 *     if hit or !(t < dist_max): the pack retires (active = 0) with its state frozen
 *     otherwise dist_prev = dist and n = find_depth_bound(t, curr):
 *       n == -1: the pack retires as a miss (active = 0, hit = 0)
 *       else:    if n != curr then t = entry[n];  curr = n;  x = o + d * t;  the pack is appended to the next active list
 *                with x (and pidx[curr] where pidx is given)
 * A retired pack's t and x are never touched again, so x == o + d * t holds bitwise for every pack. This is a stated
 * deviation: the reference's `t += dist` is unmasked, so a hit ray's reported depth keeps drifting by its last dist on every
 * later iteration. hit and x are unaffected by it. A NaN or +inf sdf retires the pack without a hit (no comparison holds).
 *
 * shacira_sphere_trace_step does all of this in one launch for the num_active packs named by active_in [num_active]
 * (slot j: pack active_in[j], its value sdf[j]); one lane per slot. Survivors are appended to active_out, coords_out
 * [., 3] and (pidx != NULL) pidx_out wave by wave: one ballot and one atomic add to *count_out per wave, so the survivors of a
 * wave stay in lane order. The order of whole waves in the next list is not fixed; a pack's results do not depend on the
 * order of the list. No workgroup waits on another. *count_out must be 0 when the launch starts; the launch sets *count_next
 * (a different int32: the counter of the FOLLOWING launch) to 0, so two counters used in turn need no clearing in between.
 * num_active == 0 returns 0 and launches nothing.
 * Bounds: 0 <= P, K < 2^31 (SHACIRA_EINVAL otherwise), P <= K (a pack holds at least one nugget), num_active <= P. NULL
 * operands are refused (SHACIRA_EINVAL) before any HIP call; find_depth_bound with P == 0 returns 0 without a launch. Slots
 * that name a pack outside [0, P) are ignored. Everything runs on `stream`; no host synchronisation and no allocation.
 */
SHACIRA_API int shacira_find_depth_bound(int64_t num_packs, int64_t num_nugs, const float *query, const int32_t *curr_idxes,
                                         const int32_t *pack_end, const float *depth, int32_t *out, void *stream);
SHACIRA_API int shacira_sphere_trace_step(int64_t num_packs, int64_t num_nugs, int64_t num_active, int first_iteration,
                                          const int32_t *active_in, const float *sdf, const float *origins,
                                          const float *dirs, const float *depth, const int32_t *pack_end,
                                          const int32_t *pidx, float step_size, float min_dis, float dist_max, float *t,
                                          float *dist, float *dist_prev, int32_t *curr, float *x, uint8_t *active,
                                          uint8_t *hit, int32_t *active_out, float *coords_out, int32_t *pidx_out,
                                          int32_t *count_out, int32_t *count_next, void *stream);

/*
 * View shading (ABI 11, additive): the per-pixel passes of the reference's OfflineRenderer over the buffers a tracer left on the
 * device -- wisp/ops/geometric.py:130-155 (spherical_envmap), wisp/ops/shaders/matcap.py:20-72, wisp/offline_renderer.py:200-215
 * (shading modes and segmentation) and :276-286 (the slice colours), wisp/ops/shaders/shadow_rays.py:31-67. The reference runs
 * the matcap lookup, the shadow blur and the slice colours on the host (scipy, numpy) after a copy out. All operands are on the
 * device unless named *_host; rows of three floats are dense ([n, 3], 4-byte aligned). fp32, one rounding per operator in the
 * order written (correctly rounded / and sqrt, no fused multiply-add); a sum of three terms is (a + b) + c. One lane per pixel,
 * no atomics, no allocation, no synchronisation: everything runs on `stream`, is capturable, and two calls return the same bits.
 * Not differentiable. Common validation, before any HIP call: n < 0, an unknown mode or bad sizes return SHACIRA_EINVAL; then
 * n == 0 returns 0 with nothing enqueued, whatever the pointers; then a NULL required operand returns SHACIRA_EINVAL.
 *
 * shacira_shade_view(n, mode, normal, dirs, hit, mm_host, tex, mh, mw, mc, rgb, uv_out, rgb8_out)
 *   normal    fp32 [n, 3] in/out (read by NORMAL and MATCAP; written only where the segmentation applies)
 *   dirs      fp32 [n, 3], the rays' directions (MATCAP only; may be NULL otherwise)
 *   hit       uint8 [n] or NULL (no segmentation)
 *   mm_host   9 floats ON THE HOST, row-major 3x3, read during the call, or NULL
 *   tex       uint8 [mh, mw, mc], row-major as PIL gives it, mc 3 or 4, mh, mw in 2 .. 32768 (scipy's interpolator needs two grid
 *             points per axis: 1 is refused). MATCAP with tex == NULL is the coordinates-only form: rgb, rgb8_out and hit must
 *             be NULL and uv_out given, and the call is spherical_envmap for device tensors; mh, mw, mc are then ignored
 *   rgb       fp32 [n, 3] in/out: read by RB, overwritten by the other modes
 *   uv_out    fp32 [n, 2], 8-byte aligned, or NULL; MATCAP only
 *   rgb8_out  uint8 [n, 3] or NULL: per channel v = rgb * 255, 0 for v <= 0 or NaN, 255 for v >= 255, else v truncated
 *   SHACIRA_SHADE_MATCAP, with n the normal and d the direction:
 *     v_i = (d_x mm[3i] + d_y mm[3i+1]) + d_z mm[3i+2]   (v = d without mm: the reference's dirs @ mm^T)
 *     v_z = -v_z;  p = 2 ((n_x v_x + n_y v_y) + n_z v_z);  r = v - p n;  r_z = r_z - 1
 *     m = 2 sqrt((r_x^2 + r_y^2) + r_z^2);  uv = 1 - (r_xy / m + 0.5);  uv = clamp to [0, 1] with NaN -> 0
 *     (a zero normal against d = (0, 0, -1) gives m = 0, 0 / 0 and uv = (0, 0); a NaN normal gives uv = (0, 0))
 *     x = u (mw - 1), x0 = min(floor x, mw - 2), fx = x - x0, the same in y with v and mh; with T the four texels as floats
 *     c = (((1-fx)(1-fy) T[y0][x0] + fx (1-fy) T[y0][x0+1]) + (1-fx) fy T[y0+1][x0]) + fx fy T[y0+1][x0+1]) / 255
 *     for the first three channels: scipy's RegularGridInterpolator over linspace(0, 1, mw) x linspace(0, 1, mh), which the
 *     reference builds per call on the host
 *   SHACIRA_SHADE_NORMAL: rgb = (normal + 1) / 2.      SHACIRA_SHADE_RB: rgb is kept.
 *   Then, where hit is given and hit[i] == 0: normal[i] = (1, 1, 1) and rgb[i] = (1, 1, 1), whatever they held.
 *   SHACIRA_EINVAL also for: mc outside {3, 4} or mh, mw out of range with tex; uv_out outside MATCAP; NULL normal (NORMAL,
 *   MATCAP), dirs (MATCAP), rgb (every form but coordinates-only); a misaligned uv_out.
 *
 * shacira_shadow_rays(n, origins, dirs, light_host, min_y, seed, depth, xyz, normal, hit, so, sd, light_hit, plane_hit)
 *   The ground plane y = min_y and one shadow ray per pixel towards the point light light_host[3] (on the host). origins, dirs
 *   fp32 [n, 3]; depth fp32 [n], xyz and normal fp32 [n, 3], hit uint8 [n] are updated in place; so, sd fp32 [n, 3] and
 *   light_hit, plane_hit uint8 [n] are overwritten. With o, d the ray:
 *     rate = -d_y;  plane_t = (o_y - min_y) / rate
 *     plane_hit = plane_t > 0 && plane_t < 500 && plane_t < depth      (NaN and the infinities of rate == 0 compare false;
 *                                                                       the reference's |rate| < 1e-5 line changes nothing)
 *     where plane_hit: hit = 0, depth = plane_t, xyz_k = o_k + d_k plane_t, normal = (0, 1, 0)
 *     so_k = xyz_k + 0.01f normal_k
 *     x_k = (light_k + 0.01f g_k) - so_k;  sd = x / max(sqrt((x_0^2 + x_1^2) + x_2^2), 1e-12f)
 *     light_hit = ((sd_0 normal_0 + sd_1 normal_1) + sd_2 normal_2) > 0
 *   g: three standard normals of ray i from Philox4x32-10 with counter (low word of i, high word of i, 0x53484457, 0) and the
 *   key (low, high word of seed), by the Box-Muller step of shacira_mesh_sample: g_0 = r0 cos, g_1 = r0 sin, g_2 = r1 cos.
 *   shacira_mesh_sample's counters hold 0 or 1 in the third word, so a shadow seed never replays a dataset's samples.
 *
 * shacira_shadow_apply(H, W, C, occluded, light_hit, shadow_out, rgb, workspace, workspace_bytes)
 *   occluded, light_hit uint8 [H W]; shadow_out uint8 [H W], overwritten, must not overlap the two inputs (any shared byte
 *   returns SHACIRA_EINVAL); rgb fp32 [H W, C] in place, C 3 or 4 (16-byte aligned for 4; the fourth channel keeps its bits);
 *   1 <= H, W < 2^30 and H W < 2^31 (the reflect period 2 H or 2 W is an int), otherwise SHACIRA_EINVAL.
 *     s = occluded && light_hit -> shadow_out;  map = clamp((1 - s) + 0.7, 0, 1)                       (1 or 0.7)
 *     taps w[k] = exp(-k^2 / 8) / sum, k = -8 .. 8, normalised in fp64 and rounded to fp32: scipy.ndimage.gaussian_filter
 *     (sigma = 2, truncate 4: radius SHACIRA_SHADOW_BLUR_RADIUS = 8)
 *     one axis: out[i] = w[0] v[i], then for k = 1 .. 8 in turn out[i] = out[i] + w[k] (v[i - k] + v[i + k])
 *     axis 0 (down the columns) into the workspace, then axis 1 on that; v[j] outside the image is read through scipy's
 *     mode='reflect' (d c b a | a b c d | d c b a) continued periodically with period 2 n, so H or W below 9 work
 *     rgb[., :3] = rgb[., :3] * blurred
 *   workspace: shacira_shadow_apply_workspace_bytes(H, W) = 4 H W bytes (0 for invalid sizes), 4-byte aligned; a missing or
 *   short one returns SHACIRA_EWORKSPACE. Two launches.
 *
 * shacira_sdf_slice_colors(n, d, vis): d fp32 [n] -> vis fp32 [n, 3], as numpy computes on a float32 array:
 *     dd = clip((d + 1) / 2, 0, 1);  blue = clip((dd - 0.5) 2, 0, 1);  yellow = 1 - blue            (clip keeps a NaN)
 *     vis = ((0 + yellow 0.4f) + 0.2f, (0 + yellow 0.3f) + 0.2f, (blue + yellow 0) + 0.2f)
 *     dd - 0.5 < 0                                        -> vis = (1, 0.38f, 0)
 *     |dd - (float)(0.02 i)| < (float)0.0015, any i in 0 .. 49  -> vis = 0.8f        (0.02 i formed in double, rounded once)
 *     |dd - 0.5| < (float)0.004                           -> vis = 0
 *   later rules overwrite earlier ones; a NaN d gives a NaN row. The reference accumulates vis in a float64 array: its colours
 *   differ from these by the fp32 rounding of three operations.
 *
 * Where the reference is not followed (wisp/ops/shaders/shadow_rays.py, wisp/offline_renderer.py):
 *   - it normalises the shadow directions over the RAY axis and keeps row [0] (F.normalize(dim=1)[0] of an [n, 3] tensor is
 *     one ray's vector); here every ray's direction is normalised on its own;
 *   - it blurs shadow_map[..., 0] of a flat [n] array (an index error); here the blur runs over the [H, W] view, so the
 *     caller must hold n == H W;
 *   - its jitter comes from the torch generator; here it is a function of (seed, ray index);
 *   - its ambient-occlusion block reads an undefined name whenever shadows are on: ambient occlusion is not built.
 */
#define SHACIRA_SHADE_RB 0
#define SHACIRA_SHADE_NORMAL 1
#define SHACIRA_SHADE_MATCAP 2
#define SHACIRA_SHADE_MAX_TEX 32768
#define SHACIRA_SHADOW_BLUR_RADIUS 8
SHACIRA_API int shacira_shade_view(int64_t n, int mode, float *normal, const float *dirs, const uint8_t *hit,
                                   const float *mm_host, const uint8_t *tex, int mh, int mw, int mc, float *rgb, float *uv_out,
                                   uint8_t *rgb8_out, void *stream);
SHACIRA_API int shacira_shadow_rays(int64_t n, const float *origins, const float *dirs, const float *light_host, float min_y,
                                    uint64_t seed, float *depth, float *xyz, float *normal, uint8_t *hit, float *so, float *sd,
                                    uint8_t *light_hit, uint8_t *plane_hit, void *stream);
SHACIRA_API size_t shacira_shadow_apply_workspace_bytes(int64_t height, int64_t width);
SHACIRA_API int shacira_shadow_apply(int64_t height, int64_t width, int channels, const uint8_t *occluded,
                                     const uint8_t *light_hit, uint8_t *shadow_out, float *rgb, void *workspace,
                                     size_t workspace_bytes, void *stream);
SHACIRA_API int shacira_sdf_slice_colors(int64_t n, const float *d, float *vis, void *stream);

/*
 * Diagnostics: one streaming pass over `bytes` (a multiple of 16; 16-byte aligned buffers) with the access shape of the
 * hash-grid kernels -- 16 bytes per lane, 8 in flight, non-temporal. kind 0 = read `src` (`dst` may be NULL or a 4-byte
 * scratch word), 1 = write `dst`, 2 = copy `src` -> `dst`. bench.py times it for `roofline.measured_stream_rates`.
 */
SHACIRA_API int shacira_stream_probe(int kind, const void *src, void *dst, size_t bytes, void *stream);

/*
 * Tunables (for benchmarking and A/B only). Process-wide atomics; every entry point takes ONE snapshot of them when it is
 * entered and uses that for the whole call (its workspace-size check included), so changing an option from another thread
 * never makes a running call inconsistent -- it applies to calls entered later. Unknown names / values -> SHACIRA_EINVAL.
 *   "fwd_variant": -1 (default) = measured rule; 0 = one gather per corner, the reference's kernel shape (any even F);
 *               3 = lane pairs, sample-major; 6 = one level per XCD + level-major staging; 8 = cell-sorted forward;
 *               9 = tables whose levels fit LDS images (groups of levels resident in LDS; refused silently, i.e. the rule
 *               applies, when a level does not fit).
 *   "bwd_variant": -1 (default) = by batch size; 0 = scattered atomics (the reference's design); 1 = binned.
 *   "bin_batch_mib": cap (MiB) of the backward's item array; larger batches are processed in sub-batches.
 *   "bin_acc_kib": LDS accumulator image per consumer workgroup: 64, 128, or 0 = chosen from the batch size (default).
 *   "bwd_compact": 1 (default) = dense levels travel as one item per sample (3-D: z-slab buckets, two slots; 2-D: line-slab
 *               buckets, one slot), 0 = pair items.
 *   "mlp_variant": -1 (default) = decoder MLPs on the fp32 matrix cores wherever instantiated, 0 = VALU kernels.
 *   "tiled": -1 (default) = the cell-sorted forward (hashgrid_tiled.hip) for batches where it measured faster (tables
 *            > 8 MB; 3-D: from 2^18 samples for F = 2, 80 K for F = 4; 2-D: from 192 K), 0 = never, 1 = whenever the shape
 *            allows it. "fwd_variant" 8 also forces it; other explicit variants exclude it.
 *   "tiled_lc_fwd": its number of coarse levels, -1 (default) = planner's choice.
 *   "bwd_fork": 1 (default) = large batches with LDS-resident ("direct") levels zero the table and accumulate those levels
 *               on a library-owned side stream, forked from and joined back into the caller's stream with events (stream
 *               semantics unchanged, capturable); 0 = one stream.
 *   "bwd_persistent": 1 (default) = the backward's last pass runs as persistent workgroups that fetch their work units from a
 *               counter (batches >= 2^17 samples); 0 = one workgroup per unit.
 *   "bwd_selective_zero": 1 (default) = the backward zeroes only the gradient rows its last pass does not overwrite with
 *               plain stores (all rows outside the hashed levels, plus hashed buckets that received 0 or several work
 *               units); 0 = the whole table first. Same result either way.
 *   "coord_variant": coordinate backward: -1 (default) = lane pairs over the plan's sorted records for 3-D calls that bring a
 *               plan (F = 2 / 4, fp32 / fp16), one lane per sample otherwise; 0 = one lane per sample; 3 = lane pairs;
 *               8 = lane pairs over the plan's records (lane pairs when the call has no plan). Same bits either way.
 *   "triplane_layout": triplane forward: -1 (default) = the measured rule, 0 = gathers from the NCHW parameters, 1 = one
 *               transpose into an HWC copy in the workspace first (profiles/triplane.md). Same bits either way.
 * (ABI 7 removed "bwd_fuse", "bwd_groups", "bwd_rows", "bwd_direct_side" and forward variants 1, 2, 4, 5, 7 -- code paths
 * that measured slower in rounds 1-2; they are recorded by git hash in profiles/.)
 */
SHACIRA_API int shacira_set_option(const char *name, int value);
SHACIRA_API int shacira_get_option(const char *name);

#ifdef __cplusplus
}
#endif
#endif /* SHACIRA_HIP_H */
