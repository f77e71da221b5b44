// api.hip -- the extern "C" entry points declared in include/shacira_hip.h: argument validation, level-table
// construction and dispatch. No allocation, no synchronisation, no global mutable state besides the tunables (atomics,
// snapshotted once per call).
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "internal.h"

namespace shacira {

// ---- tunables: process-wide atomics, one snapshot per API call (internal.h) ------------------------------------------
struct OptionSlot {
    const char *name;
    int Options::*field;
    int lo, hi;           // accepted range (inclusive)
    std::atomic<int> value;
};
static OptionSlot g_slots[] = {
    {"fwd_variant", &Options::fwd_variant, -1, 9, {-1}},
    {"bwd_variant", &Options::bwd_variant, -1, 1, {-1}},
    {"mlp_variant", &Options::mlp_variant, -1, 1, {-1}},
    {"bwd_compact", &Options::bwd_compact, 0, 1, {1}},
    {"bwd_selective_zero", &Options::bwd_selective_zero, 0, 1, {1}},
    {"bwd_persistent", &Options::bwd_persistent, 0, 1, {1}},
    {"bwd_fork", &Options::bwd_fork, 0, 1, {1}},
    {"bwd_run_pad", &Options::bwd_run_pad, 0, 1, {1}},
    {"bwd_item12", &Options::bwd_item12, -1, 1, {-1}},
    {"bin_acc_kib", &Options::bin_acc_kib, 0, 128, {0}},
    {"bin_batch_mib", &Options::bin_batch_mib, 1, 1 << 20, {1536}},
    {"tiled", &Options::tiled, -1, 1, {-1}},
    {"tiled_lc_fwd", &Options::tiled_lc_fwd, -1, SHACIRA_MAX_LODS, {-1}},
    {"bwd_brick", &Options::bwd_brick, -1, 1, {-1}},
    {"bwd_brick_lo", &Options::bwd_brick_lo, -1, SHACIRA_MAX_LODS, {-1}},
    {"bwd_brick_hi", &Options::bwd_brick_hi, -1, SHACIRA_MAX_LODS, {-1}},
    {"bwd_brick_fork", &Options::bwd_brick_fork, 0, 2, {2}},
    {"bwd_brick_span", &Options::bwd_brick_span, 0, 64, {0}},
    {"fwd_direct", &Options::fwd_direct, -1, 1, {-1}},
    {"bwd_ext_fork", &Options::bwd_ext_fork, 0, 1, {1}},
    {"coord_variant", &Options::coord_variant, -1, 8, {-1}},
    {"triplane_layout", &Options::triplane_layout, -1, 1, {-1}},
};
static thread_local Options tl_options;
const Options &opt() { return tl_options; }
void options_snapshot() {
    for (OptionSlot &sl : g_slots) tl_options.*(sl.field) = sl.value.load(std::memory_order_relaxed);
}
static bool option_value_ok(const OptionSlot &sl, int v) {
    if (v < sl.lo || v > sl.hi) return false;
    if (!std::strcmp(sl.name, "fwd_variant")) return v == -1 || v == 0 || v == 3 || v == 6 || v == 8 || v == 9;
    if (!std::strcmp(sl.name, "coord_variant")) return v == -1 || v == 0 || v == 3 || v == 8;
    if (!std::strcmp(sl.name, "bin_acc_kib")) return v == 0 || v == 64 || v == 128;
    return true;
}

static int build_level_table(int dim, int num_lods, int feature_dim, int bw, const int32_t *res_host,
                             int64_t table_rows, LevelTable &lt) {
    if (dim != 2 && dim != 3) return SHACIRA_EINVAL;
    if (num_lods < 1 || num_lods > SHACIRA_MAX_LODS) return SHACIRA_EINVAL;
    if (feature_dim < 1) return SHACIRA_EINVAL;
    if (feature_dim % 2 == 1) return SHACIRA_EODD;
    if (bw < 1 || bw > 30) return SHACIRA_EINVAL;  // int32_t codebook_size = pow(2, bw), .cpp:56
    if (!res_host || table_rows < 0) return SHACIRA_EINVAL;
    std::memset(&lt, 0, sizeof(lt));
    const int32_t cs = (int32_t)std::pow(2.0, (double)bw);
    for (int l = 0; l < num_lods; ++l) {
        const int32_t r = res_host[l];
        if (r < 1) return SHACIRA_EINVAL;
        lt.res[l] = r;
        lt.hi[l] = (float)((double)r - 1.0 - 1e-5);  // `resolution-1-1e-5` narrowed at the clamp() call
        lt.dense[l] = level_is_dense(dim, r, cs) ? 1 : 0;
    }
    lt.mask = (uint32_t)cs - 1u;
    lt.num_lods = num_lods;
    lt.feature_dim = feature_dim;
    lt.table_rows = table_rows;
    lt.level_begin = 0;
    lt.level_end = num_lods;
    lt.stage_flags = 0;
    return 0;
}

// What a hash-grid entry point knows once the eight shape arguments every one of them begins with are resolved.
struct GridCall {
    LevelTable lt;
    int dim, dtype;
    int64_t n;
    bool sorts;   // the forward cell-sorts this shape, so its plan exists (shacira_hashgrid_plan_bytes > 0): THE rule, once
};
enum GridAccept { kShapeOnly, kNoF64, kAnyFloat };   // the scalar types an entry takes; kShapeOnly: judged later or never

// dtype, then the batch size: the second stage of resolve_grid, on its own for the entry that judges other things first
static int grid_batch_ok(const GridCall &c, GridAccept accept) {
    if (c.dtype != SHACIRA_F32 && c.dtype != SHACIRA_F16 && !(c.dtype == SHACIRA_F64 && accept == kAnyFloat)) return SHACIRA_EDTYPE;
    return c.n < 0 ? SHACIRA_EINVAL : 0;
}

// options snapshot, level table, plan rule; unless kShapeOnly, dtype and batch size. Error codes in the order listed.
static int resolve_grid(int dim, int64_t num_coords, int num_lods, int feature_dim, int bw, const int32_t *res_host,
                        int64_t table_rows, int dtype, GridAccept accept, GridCall &c) {
    options_snapshot();
    const int rc = build_level_table(dim, num_lods, feature_dim, bw, res_host, table_rows, c.lt);
    if (rc) return rc;
    c.dim = dim;
    c.dtype = dtype;
    c.n = num_coords;
    c.sorts = dtype != SHACIRA_F64 && table_rows > 0 && tiled_supported(dim, dtype, c.lt, num_coords);
    return accept == kShapeOnly ? 0 : grid_batch_ok(c, accept);
}

// A caller's plan buffer: the plan of a shape whose forward sorts nothing does not exist, so such a buffer is ignored (`plan`
// is NULL afterwards); one that is used holds sample_plan_bytes.
template <typename P>
static int caller_plan(const GridCall &c, P *&plan, size_t plan_bytes) {
    if (plan != nullptr && !c.sorts) plan = nullptr;
    return plan != nullptr && plan_bytes < sample_plan_bytes(c.dim, c.n) ? SHACIRA_EWORKSPACE : 0;
}

}  // namespace shacira

using namespace shacira;

extern "C" {

int shacira_abi_version(void) { return SHACIRA_ABI_VERSION; }

const char *shacira_strerror(int code) {
    switch (code) {
        case 0: return "success";
        case SHACIRA_EINVAL: return "shacira: invalid argument (dim/sizes/bitwidth/null pointer)";
        case SHACIRA_EDTYPE: return "shacira: unsupported scalar type or operator shape";
        case SHACIRA_EODD: return "The codebook feature dimension needs to be a multiple of 2.";
        case SHACIRA_EWORKSPACE: return "shacira: workspace too small";
        default: break;
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "shacira: unknown error";
}

int shacira_set_option(const char *name, int value) {
    if (!name) return SHACIRA_EINVAL;
    for (OptionSlot &sl : g_slots) {
        if (std::strcmp(name, sl.name)) continue;
        if (!option_value_ok(sl, value)) return SHACIRA_EINVAL;
        sl.value.store(value, std::memory_order_relaxed);
        return 0;
    }
    return SHACIRA_EINVAL;
}

int shacira_get_option(const char *name) {
    if (!name) return SHACIRA_EINVAL;
    for (OptionSlot &sl : g_slots)
        if (!std::strcmp(name, sl.name)) return sl.value.load(std::memory_order_relaxed);
    return SHACIRA_EINVAL;
}

size_t shacira_hashgrid_forward_workspace_bytes(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                int codebook_bitwidth, const int32_t *resolutions_host,
                                                int64_t table_rows, int dtype) {
    GridCall c;
    if (resolve_grid(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host, table_rows, dtype,
                     kShapeOnly, c)) return 0;
    return hashgrid_forward_workspace(dim, dtype, c.lt, num_coords);
}

int shacira_hashgrid_forward(int dim, int64_t num_coords, int num_lods, int feature_dim, int codebook_bitwidth,
                             const int32_t *resolutions_host, const int32_t *codebook_first_idx, int64_t table_rows,
                             const float *coords, const void *codebook, int dtype, void *feats, void *workspace,
                             size_t workspace_bytes, void *stream) {
    return shacira_hashgrid_forward_planned(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host,
                                            codebook_first_idx, table_rows, coords, codebook, dtype, feats, nullptr, 0, 0,
                                            workspace, workspace_bytes, stream);
}

size_t shacira_hashgrid_plan_bytes(int dim, int64_t num_coords, int num_lods, int feature_dim, int codebook_bitwidth,
                                   const int32_t *resolutions_host, int64_t table_rows, int dtype) {
    GridCall c;
    if (resolve_grid(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host, table_rows, dtype,
                     kShapeOnly, c)) return 0;
    return c.sorts ? sample_plan_bytes(dim, num_coords) : 0;
}

int shacira_hashgrid_forward_planned(int dim, int64_t num_coords, int num_lods, int feature_dim, int codebook_bitwidth,
                                     const int32_t *resolutions_host, const int32_t *codebook_first_idx, int64_t table_rows,
                                     const float *coords, const void *codebook, int dtype, void *feats, void *plan,
                                     size_t plan_bytes, int plan_flags, void *workspace, size_t workspace_bytes,
                                     void *stream) {
    GridCall c;
    if (const int rc = resolve_grid(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host, table_rows,
                                    dtype, kAnyFloat, c)) return rc;
    if (num_coords == 0) return 0;
    if (!codebook_first_idx || !coords || !codebook || !feats) return SHACIRA_EINVAL;
    const bool brought = plan != nullptr;   // SHACIRA_PLAN_READY is judged by what the caller brought, used or ignored
    if (caller_plan(c, plan, plan_bytes)) return SHACIRA_EWORKSPACE;
    // (a call whose plan buffer is used needs shacira_hashgrid_plan_bytes less than the workspace query says)
    const size_t need = hashgrid_forward_workspace(dim, dtype, c.lt, num_coords, plan != nullptr);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SHACIRA_EWORKSPACE;
    const bool ready = (plan_flags & SHACIRA_PLAN_READY) != 0;
    if ((plan_flags & ~SHACIRA_PLAN_READY) != 0 || (ready && !brought)) return SHACIRA_EINVAL;
    return (int)hashgrid_forward_dispatch(dim, dtype, c.lt, codebook_first_idx, coords, codebook, feats, workspace,
                                          num_coords, (hipStream_t)stream, plan, ready);
}

int shacira_hashgrid_debug_corners(int dim, int64_t num_coords, int num_lods, int codebook_bitwidth,
                                   const int32_t *resolutions_host, const float *coords, int32_t *corner_rows,
                                   float *corner_weights, void *stream) {
    GridCall c;   // (corners depend on no table: two features, no rows, no scalar type)
    if (const int rc = resolve_grid(dim, num_coords, num_lods, 2, codebook_bitwidth, resolutions_host, 0, SHACIRA_F32,
                                    kShapeOnly, c)) return rc;
    if (num_coords < 0 || num_coords * (int64_t)num_lods >= ((int64_t)1 << 31) * 256) return SHACIRA_EINVAL;
    if (num_coords > 0 && (!coords || (!corner_rows && !corner_weights))) return SHACIRA_EINVAL;
    return (int)hashgrid_debug_corners(dim, c.lt, coords, num_coords, corner_rows, corner_weights, (hipStream_t)stream);
}

size_t shacira_hashgrid_backward_workspace_bytes(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                 int codebook_bitwidth, const int32_t *resolutions_host,
                                                 int64_t table_rows, int dtype) {
    GridCall c;
    if (resolve_grid(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host, table_rows, dtype,
                     kShapeOnly, c)) return 0;
    return hashgrid_backward_workspace(dim, dtype, c.lt, num_coords);
}

// the body of the three backward entry points
static int backward_call(int dim, int64_t num_coords, int num_lods, int feature_dim, int codebook_bitwidth,
                         const int32_t *resolutions_host, const int32_t *codebook_first_idx, int64_t table_rows,
                         const float *coords, const void *grad_output, int dtype, void *grad_codebook, int level_begin,
                         int level_end, int flags, const void *plan, size_t plan_bytes, void *workspace,
                         size_t workspace_bytes, void *stream) {
    GridCall c;
    // (kShapeOnly: the level range and its rules are judged before the scalar type)
    if (const int rc = resolve_grid(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host, table_rows,
                                    dtype, kShapeOnly, c)) return rc;
    if (level_begin < 0 || level_end > num_lods || level_begin >= level_end) return SHACIRA_EINVAL;
    const bool partial = !(level_begin == 0 && level_end == num_lods);
    // level ranges: fp32 tables, and (round 4) fp16 tables without the staged-gradient flags -- each call then converts its own
    // rows of the fp32 accumulation image only; double tables take whole calls
    if (partial && dtype == SHACIRA_F64) return SHACIRA_EDTYPE;
    if (dtype == SHACIRA_F16 && (flags & (SHACIRA_BWD_STAGE_ALL_LEVELS | SHACIRA_BWD_REUSE_STAGED)) != 0) return SHACIRA_EDTYPE;
    c.lt.level_begin = level_begin;
    c.lt.level_end = level_end;
    c.lt.stage_flags = flags & (SHACIRA_BWD_STAGE_ALL_LEVELS | SHACIRA_BWD_REUSE_STAGED);
    if (const int rc = grid_batch_ok(c, kAnyFloat)) return rc;
    if (!grad_codebook) return SHACIRA_EINVAL;
    if (num_coords > 0 && (!codebook_first_idx || !coords || !grad_output)) return SHACIRA_EINVAL;
    if (caller_plan(c, plan, plan_bytes)) return SHACIRA_EWORKSPACE;
    // a planned call is sized by what it runs: shacira_hashgrid_backward_planned_workspace_bytes when its brick pass takes the
    // coarse levels (16-byte aligned grad_output), the plain size otherwise. The dispatcher checks it, before it launches
    // anything, with the call it resolved for the launch.
    bool too_small = false;
    const hipError_t e = hashgrid_backward_dispatch(dim, dtype, c.lt, codebook_first_idx, coords, grad_output, grad_codebook,
                                                    workspace, workspace_bytes, num_coords, (hipStream_t)stream, plan, &too_small);
    return too_small ? SHACIRA_EWORKSPACE : (int)e;
}

int shacira_hashgrid_backward(int dim, int64_t num_coords, int num_lods, int feature_dim, int codebook_bitwidth,
                              const int32_t *resolutions_host, const int32_t *codebook_first_idx, int64_t table_rows,
                              const float *coords, const void *grad_output, int dtype, void *grad_codebook,
                              void *workspace, size_t workspace_bytes, void *stream) {
    return shacira_hashgrid_backward_levels(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host,
                                            codebook_first_idx, table_rows, coords, grad_output, dtype, grad_codebook,
                                            0, num_lods, 0, workspace, workspace_bytes, stream);
}

size_t shacira_hashgrid_backward_planned_workspace_bytes(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                         int codebook_bitwidth, const int32_t *resolutions_host,
                                                         int64_t table_rows, int dtype) {
    GridCall c;
    if (resolve_grid(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host, table_rows, dtype,
                     kShapeOnly, c)) return 0;
    if (!c.sorts) return hashgrid_backward_workspace(dim, dtype, c.lt, num_coords);   // no plan for this shape: the plain call
    return hashgrid_backward_workspace_planned(dim, dtype, c.lt, num_coords, true);
}

int shacira_hashgrid_backward_planned(int dim, int64_t num_coords, int num_lods, int feature_dim, int codebook_bitwidth,
                                      const int32_t *resolutions_host, const int32_t *codebook_first_idx, int64_t table_rows,
                                      const float *coords, const void *grad_output, int dtype, void *grad_codebook,
                                      const void *plan, size_t plan_bytes, void *workspace, size_t workspace_bytes,
                                      void *stream) {
    return backward_call(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host, codebook_first_idx,
                         table_rows, coords, grad_output, dtype, grad_codebook, 0, num_lods, 0, plan, plan_bytes, workspace,
                         workspace_bytes, stream);
}

int shacira_hashgrid_backward_levels(int dim, int64_t num_coords, int num_lods, int feature_dim, int codebook_bitwidth,
                                     const int32_t *resolutions_host, const int32_t *codebook_first_idx,
                                     int64_t table_rows, const float *coords, const void *grad_output, int dtype,
                                     void *grad_codebook, int level_begin, int level_end, int flags, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    return backward_call(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host, codebook_first_idx,
                         table_rows, coords, grad_output, dtype, grad_codebook, level_begin, level_end, flags, nullptr, 0,
                         workspace, workspace_bytes, stream);
}

size_t shacira_hashgrid_coords_backward_workspace_bytes(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                        int codebook_bitwidth, const int32_t *resolutions_host,
                                                        int64_t table_rows, int dtype) {
    return 0;   // every variant is a pure gather (the ABI keeps the argument for later variants)
}

int shacira_hashgrid_coords_backward(int dim, int64_t num_coords, int num_lods, int feature_dim, int codebook_bitwidth,
                                     const int32_t *resolutions_host, const int32_t *codebook_first_idx, int64_t table_rows,
                                     const float *coords, const void *codebook, const void *grad_output, int dtype,
                                     float *grad_coords, const void *plan, size_t plan_bytes, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    GridCall c;
    if (const int rc = resolve_grid(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host, table_rows,
                                    dtype, kAnyFloat, c)) return rc;
    if (num_coords == 0) return 0;
    if (!codebook_first_idx || !coords || !codebook || !grad_output || !grad_coords) return SHACIRA_EINVAL;
    const size_t need = shacira_hashgrid_coords_backward_workspace_bytes(dim, num_coords, num_lods, feature_dim,
                                                                         codebook_bitwidth, resolutions_host, table_rows,
                                                                         dtype);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SHACIRA_EWORKSPACE;
    if (caller_plan(c, plan, plan_bytes)) return SHACIRA_EWORKSPACE;
    return (int)hashgrid_coord_grad_dispatch(dim, dtype, c.lt, codebook_first_idx, coords, codebook, grad_output, grad_coords,
                                             num_coords, (hipStream_t)stream, plan);
}

// fp16 tables: the fp32 image grad_codebook is accumulated in (used only by calls that ask for grad_codebook)
static size_t coords_backward2_workspace(const GridCall &c) {
    return c.dtype == SHACIRA_F16 ? (size_t)c.lt.table_rows * (size_t)c.lt.feature_dim * sizeof(float) : 0;
}

size_t shacira_hashgrid_coords_backward2_workspace_bytes(int dim, int64_t num_coords, int num_lods, int feature_dim,
                                                         int codebook_bitwidth, const int32_t *resolutions_host,
                                                         int64_t table_rows, int dtype) {
    GridCall c;
    if (resolve_grid(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host, table_rows, dtype,
                     kShapeOnly, c)) return 0;
    return coords_backward2_workspace(c);
}

int shacira_hashgrid_coords_backward2(int dim, int64_t num_coords, int num_lods, int feature_dim, int codebook_bitwidth,
                                      const int32_t *resolutions_host, const int32_t *codebook_first_idx, int64_t table_rows,
                                      const float *coords, const void *codebook, const void *grad_output,
                                      const float *grad_grad_coords, int dtype, void *grad_grad_output, void *grad_codebook,
                                      float *grad_coords, const void *plan, size_t plan_bytes, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    GridCall c;   // (kNoF64: double tables are first order only)
    if (const int rc = resolve_grid(dim, num_coords, num_lods, feature_dim, codebook_bitwidth, resolutions_host, table_rows,
                                    dtype, kNoF64, c)) return rc;
    if (!grad_grad_output && !grad_codebook && !grad_coords) return SHACIRA_EINVAL;
    if (num_coords > 0) {
        if (!codebook_first_idx || !coords || !grad_grad_coords) return SHACIRA_EINVAL;
        if (!codebook && (grad_grad_output || grad_coords)) return SHACIRA_EINVAL;
        if (!grad_output && (grad_codebook || grad_coords)) return SHACIRA_EINVAL;
        if (grad_codebook && dtype == SHACIRA_F16 && table_rows > 0 &&
            (!workspace || workspace_bytes < coords_backward2_workspace(c))) return SHACIRA_EWORKSPACE;
        if (caller_plan(c, plan, plan_bytes)) return SHACIRA_EWORKSPACE;
    }
    return (int)hashgrid_coord_grad2_dispatch(dim, dtype, c.lt, codebook_first_idx, coords, codebook, grad_output,
                                              grad_grad_coords, grad_grad_output, grad_codebook, grad_coords, workspace,
                                              num_coords, (hipStream_t)stream, plan);
}

// ---- triplanes ---------------------------------------------------------------------------------------------------------
static int triplane_args(int64_t num_coords, int num_lods, const int32_t *lods_host, int feature_dim, TriplaneArgs &a) {
    if (num_coords < 0 || num_coords > (int64_t)INT32_MAX) return SHACIRA_EINVAL;
    if (num_lods < 1 || num_lods > SHACIRA_TRIPLANE_MAX_LODS || !lods_host) return SHACIRA_EINVAL;
    if (feature_dim < 1 || feature_dim > SHACIRA_TRIPLANE_MAX_FDIM) return SHACIRA_EINVAL;
    std::memset(&a, 0, sizeof(a));
    a.num_lods = num_lods;
    a.fdim = feature_dim;
    for (int l = 0; l < num_lods; ++l) {
        if (lods_host[l] < 0 || lods_host[l] > SHACIRA_TRIPLANE_MAX_LOD) return SHACIRA_EINVAL;
        a.side[l] = (1 << lods_host[l]) + 1;
    }
    return 0;
}

static int triplane_pointers(int num_lods, const float *const *host, TriplaneArgs &a, bool grad) {
    if (!host) return SHACIRA_EINVAL;
    for (int q = 0; q < 3 * num_lods; ++q) {
        if (!host[q]) return SHACIRA_EINVAL;
        if (grad) a.grad[q] = const_cast<float *>(host[q]);
        else a.plane[q] = host[q];
    }
    return 0;
}

size_t shacira_triplane_forward_workspace_bytes(int64_t num_coords, int num_lods, const int32_t *lods_host,
                                                int feature_dim, int multiscale_sum) {
    options_snapshot();
    TriplaneArgs a;
    if (triplane_args(num_coords, num_lods, lods_host, feature_dim, a)) return 0;
    return triplane_forward_workspace(a, num_coords);
}

int shacira_triplane_forward(int64_t num_coords, int num_lods, const int32_t *lods_host, int feature_dim,
                             const float *coords, const float *const *planes_host, int multiscale_sum, float *feats,
                             void *workspace, size_t workspace_bytes, void *stream) {
    options_snapshot();
    TriplaneArgs a;
    if (int rc = triplane_args(num_coords, num_lods, lods_host, feature_dim, a)) return rc;
    if (multiscale_sum != 0 && multiscale_sum != 1) return SHACIRA_EINVAL;
    if (num_coords == 0) return 0;
    if (!coords || !feats) return SHACIRA_EINVAL;
    if (int rc = triplane_pointers(num_lods, planes_host, a, false)) return rc;
    const size_t need = triplane_forward_workspace(a, num_coords);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SHACIRA_EWORKSPACE;
    return (int)triplane_forward_dispatch(a, coords, multiscale_sum, feats, workspace, num_coords, (hipStream_t)stream);
}

size_t shacira_triplane_backward_workspace_bytes(int64_t num_coords, int num_lods, const int32_t *lods_host,
                                                 int feature_dim, int multiscale_sum, int flags) {
    TriplaneArgs a;
    if (triplane_args(num_coords, num_lods, lods_host, feature_dim, a)) return 0;
    if ((flags & SHACIRA_TRIPLANE_GRAD_PLANES) == 0) return 0;
    return triplane_backward_workspace(a, multiscale_sum, num_coords);
}

int shacira_triplane_backward(int64_t num_coords, int num_lods, const int32_t *lods_host, int feature_dim,
                              const float *coords, const float *const *planes_host, const float *grad_output,
                              int multiscale_sum, int flags, float *const *grad_planes_host, float *grad_coords,
                              void *workspace, size_t workspace_bytes, void *stream) {
    TriplaneArgs a;
    if (int rc = triplane_args(num_coords, num_lods, lods_host, feature_dim, a)) return rc;
    if (multiscale_sum != 0 && multiscale_sum != 1) return SHACIRA_EINVAL;
    if (flags <= 0 || (flags & ~(SHACIRA_TRIPLANE_GRAD_PLANES | SHACIRA_TRIPLANE_GRAD_COORDS)) != 0) return SHACIRA_EINVAL;
    const bool planes = (flags & SHACIRA_TRIPLANE_GRAD_PLANES) != 0;
    const bool want_coords = (flags & SHACIRA_TRIPLANE_GRAD_COORDS) != 0;
    if (planes)
        if (int rc = triplane_pointers(num_lods, const_cast<const float *const *>(grad_planes_host), a, true)) return rc;
    if (num_coords > 0) {
        if (!coords || !grad_output) return SHACIRA_EINVAL;
        if (want_coords) {
            if (!grad_coords) return SHACIRA_EINVAL;
            if (int rc = triplane_pointers(num_lods, planes_host, a, false)) return rc;
        }
    }
    const size_t need = planes ? triplane_backward_workspace(a, multiscale_sum, num_coords) : 0;
    if (need > 0 && (!workspace || workspace_bytes < need)) return SHACIRA_EWORKSPACE;
    return (int)triplane_backward_dispatch(a, coords, grad_output, multiscale_sum, planes,
                                           want_coords ? grad_coords : nullptr, workspace, num_coords,
                                           (hipStream_t)stream);
}

// ---- octree grids --------------------------------------------------------------------------------------------------------
static int octree_args(int64_t num_coords, int num_levels, const int32_t *levels_host, int feature_dim, OctreeArgs &a) {
    if (num_coords < 0 || num_coords > (int64_t)INT32_MAX) return SHACIRA_EINVAL;
    if (num_levels < 1 || num_levels > SHACIRA_OCTREE_MAX_LEVELS || !levels_host) return SHACIRA_EINVAL;
    if (feature_dim < 1 || feature_dim > SHACIRA_OCTREE_MAX_FDIM) return SHACIRA_EINVAL;
    std::memset(&a, 0, sizeof(a));
    a.num_levels = num_levels;
    a.fdim = feature_dim;
    for (int l = 0; l < num_levels; ++l) {
        if (levels_host[l] < 0 || levels_host[l] > SHACIRA_OCTREE_MAX_LEVEL) return SHACIRA_EINVAL;
        a.level[l] = levels_host[l];
    }
    return 0;
}

static int octree_rows(const int64_t *rows_host, OctreeArgs &a) {
    if (!rows_host) return SHACIRA_EINVAL;
    for (int l = 0; l < a.num_levels; ++l) {
        const int64_t side = ((int64_t)1 << a.level[l]) + 1;
        if (rows_host[l] < 0 || rows_host[l] > side * side * side) return SHACIRA_EINVAL;
        a.rows[l] = rows_host[l];
    }
    return 0;
}

static int octree_index(const void *const *corner_index_host, const void *const *occupancy_host, OctreeArgs &a) {
    if (!corner_index_host || !occupancy_host) return SHACIRA_EINVAL;
    for (int l = 0; l < a.num_levels; ++l) {
        if (!corner_index_host[l] || !occupancy_host[l]) return SHACIRA_EINVAL;
        a.corner[l] = static_cast<const uint2 *>(corner_index_host[l]);
        a.occ[l] = static_cast<const uint32_t *>(occupancy_host[l]);
    }
    return 0;
}

static int octree_tables(const float *const *tables_host, OctreeArgs &a) {
    if (!tables_host) return SHACIRA_EINVAL;
    for (int l = 0; l < a.num_levels; ++l) {
        if (!tables_host[l]) return SHACIRA_EINVAL;
        a.table[l] = tables_host[l];
    }
    return 0;
}

size_t shacira_octree_forward_workspace_bytes(int64_t num_coords, int num_levels, const int32_t *levels_host,
                                              int feature_dim, int multiscale_sum) {
    return 0;   // the forward needs none; the query keeps the calling sequence of the other operators
}

int shacira_octree_forward(int64_t num_coords, int num_levels, const int32_t *levels_host, int feature_dim,
                           const float *coords, const float *const *tables_host, const int64_t *rows_host,
                           const void *const *corner_index_host, const void *const *occupancy_host, int multiscale_sum,
                           float *feats, void *workspace, size_t workspace_bytes, void *stream) {
    OctreeArgs a;
    if (int rc = octree_args(num_coords, num_levels, levels_host, feature_dim, a)) return rc;
    if (multiscale_sum != 0 && multiscale_sum != 1) return SHACIRA_EINVAL;
    if (int rc = octree_rows(rows_host, a)) return rc;
    if (num_coords == 0) return 0;
    if (!coords || !feats) return SHACIRA_EINVAL;
    if (int rc = octree_tables(tables_host, a)) return rc;
    if (int rc = octree_index(corner_index_host, occupancy_host, a)) return rc;
    return (int)octree_forward_dispatch(a, coords, multiscale_sum, feats, num_coords, (hipStream_t)stream);
}

size_t shacira_octree_backward_workspace_bytes(int64_t num_coords, int num_levels, const int32_t *levels_host,
                                               int feature_dim, int multiscale_sum, int flags) {
    OctreeArgs a;
    if (octree_args(num_coords, num_levels, levels_host, feature_dim, a)) return 0;
    if ((flags & SHACIRA_OCTREE_GRAD_FEATURES) == 0) return 0;
    return octree_backward_workspace(a, multiscale_sum, num_coords);
}

int shacira_octree_backward(int64_t num_coords, int num_levels, const int32_t *levels_host, int feature_dim,
                            const float *coords, const float *const *tables_host, const int64_t *rows_host,
                            const void *const *corner_index_host, const void *const *occupancy_host,
                            const float *grad_output, int multiscale_sum, int flags, float *const *grad_tables_host,
                            float *grad_coords, void *workspace, size_t workspace_bytes, void *stream) {
    OctreeArgs a;
    if (int rc = octree_args(num_coords, num_levels, levels_host, feature_dim, a)) return rc;
    if (multiscale_sum != 0 && multiscale_sum != 1) return SHACIRA_EINVAL;
    if (flags <= 0 || (flags & ~(SHACIRA_OCTREE_GRAD_FEATURES | SHACIRA_OCTREE_GRAD_COORDS)) != 0) return SHACIRA_EINVAL;
    if (int rc = octree_rows(rows_host, a)) return rc;
    const bool features = (flags & SHACIRA_OCTREE_GRAD_FEATURES) != 0;
    const bool want_coords = (flags & SHACIRA_OCTREE_GRAD_COORDS) != 0;
    if (features) {
        if (!grad_tables_host) return SHACIRA_EINVAL;
        for (int l = 0; l < num_levels; ++l) {
            if (!grad_tables_host[l]) return SHACIRA_EINVAL;
            a.grad[l] = grad_tables_host[l];
        }
    }
    if (num_coords > 0) {
        if (!coords || !grad_output) return SHACIRA_EINVAL;
        if (int rc = octree_index(corner_index_host, occupancy_host, a)) return rc;
        if (want_coords) {
            if (!grad_coords) return SHACIRA_EINVAL;
            if (int rc = octree_tables(tables_host, a)) return rc;
        }
    }
    const size_t need = features ? octree_backward_workspace(a, multiscale_sum, num_coords) : 0;
    if (need > 0 && (!workspace || workspace_bytes < need)) return SHACIRA_EWORKSPACE;
    return (int)octree_backward_dispatch(a, coords, grad_output, multiscale_sum, features,
                                         want_coords ? grad_coords : nullptr, workspace, num_coords, (hipStream_t)stream);
}

// ---- mesh to signed distance -----------------------------------------------------------------------------------------------
static bool mesh_counts_ok(int64_t num_points, int64_t num_triangles) {
    return num_points >= 0 && num_triangles >= 0 && num_points <= INT32_MAX && num_triangles <= INT32_MAX;
}

size_t shacira_mesh_sdf_workspace_bytes(int64_t num_points, int64_t num_triangles) {
    if (!mesh_counts_ok(num_points, num_triangles)) return 0;
    return mesh_sdf_workspace(num_points, num_triangles);
}

int shacira_mesh_sdf(int64_t num_points, int64_t num_triangles, const float *points, const float *triangles, float *sdf,
                     void *workspace, size_t workspace_bytes, void *stream) {
    if (!mesh_counts_ok(num_points, num_triangles)) return SHACIRA_EINVAL;
    if (num_points == 0) return 0;
    if (!points || !sdf || (num_triangles > 0 && !triangles)) return SHACIRA_EINVAL;
    const size_t need = mesh_sdf_workspace(num_points, num_triangles);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SHACIRA_EWORKSPACE;
    return (int)mesh_sdf_dispatch(num_points, num_triangles, points, triangles, sdf, workspace, (hipStream_t)stream);
}

size_t shacira_mesh_closest_workspace_bytes(int64_t num_points, int64_t num_triangles, int32_t flags) {
    if (!mesh_counts_ok(num_points, num_triangles) || (flags & ~SHACIRA_MESH_CLOSEST_SIGNED)) return 0;
    return mesh_closest_workspace(num_points, num_triangles);
}

int shacira_mesh_closest(int64_t num_points, int64_t num_triangles, const float *points, const float *triangles,
                         int32_t flags, float *dist, float *hit, int32_t *tidx, void *workspace, size_t workspace_bytes,
                         void *stream) {
    if (!mesh_counts_ok(num_points, num_triangles) || (flags & ~SHACIRA_MESH_CLOSEST_SIGNED)) return SHACIRA_EINVAL;
    if (num_points == 0) return 0;
    if (!points || !dist || !hit || !tidx || (num_triangles > 0 && !triangles)) return SHACIRA_EINVAL;
    const size_t need = mesh_closest_workspace(num_points, num_triangles);
    if (!workspace || workspace_bytes < need) return SHACIRA_EWORKSPACE;
    return (int)mesh_closest_dispatch(num_points, num_triangles, points, triangles, (flags & SHACIRA_MESH_CLOSEST_SIGNED) != 0,
                                      dist, hit, tidx, workspace, (hipStream_t)stream);
}

// ---- mesh to occupancy ---------------------------------------------------------------------------------------------------
static bool voxelize_args_ok(int64_t num_triangles, int level) {
    return num_triangles >= 0 && num_triangles <= INT32_MAX && level >= 0 && level <= SHACIRA_OCTREE_MAX_LEVEL;
}

size_t shacira_mesh_voxelize_workspace_bytes(int64_t num_triangles, int level) {
    if (!voxelize_args_ok(num_triangles, level)) return 0;
    return mesh_voxelize_workspace(num_triangles);
}

int shacira_mesh_voxelize(int64_t num_triangles, const float *triangles, int level, float margin,
                          uint32_t *occupancy_words, uint8_t *occupancy_grid, void *workspace, size_t workspace_bytes,
                          void *stream) {
    if (!voxelize_args_ok(num_triangles, level) || !(margin >= 0.f) || std::isinf(margin)) return SHACIRA_EINVAL;
    if (!occupancy_words || (num_triangles > 0 && !triangles)) return SHACIRA_EINVAL;
    if (level >= 2 && ((uintptr_t)occupancy_grid & 15u)) return SHACIRA_EINVAL;     // written 16 bytes at a time
    const size_t need = mesh_voxelize_workspace(num_triangles);
    if (need > 0 && (!workspace || workspace_bytes < need)) return SHACIRA_EWORKSPACE;
    return (int)mesh_voxelize_dispatch(num_triangles, triangles, level, margin, occupancy_words, occupancy_grid, workspace,
                                       (hipStream_t)stream);
}

// ---- mesh point sampling ---------------------------------------------------------------------------------------------------
// 0: launch; 1: nothing to do (n == 0); SHACIRA_EINVAL
static int mesh_sample_args(int mode, int64_t n, int64_t index_base, uint64_t seed, uint32_t segment, const uint32_t *words,
                            int64_t num_triangles, const float *triangles, const uint32_t *cdf, float sigma,
                            int64_t num_cells, const int16_t *corners, int samples_per_cell, int cell_level,
                            const uint32_t *occupancy_words, int occupancy_level, MeshSampleArgs &a) {
    if (mode < SHACIRA_MESH_SAMPLE_SURFACE || mode > SHACIRA_MESH_SAMPLE_CELLS) return SHACIRA_EINVAL;
    if (n < 0 || n > INT32_MAX || index_base < 0 || index_base > INT64_MAX - n) return SHACIRA_EINVAL;
    const bool faces = mode == SHACIRA_MESH_SAMPLE_SURFACE || mode == SHACIRA_MESH_SAMPLE_NEAR;
    if (faces && (num_triangles < 0 || num_triangles > INT32_MAX)) return SHACIRA_EINVAL;
    if (mode == SHACIRA_MESH_SAMPLE_CELLS) {
        if (num_cells < 0 || num_cells > INT32_MAX || samples_per_cell < 1) return SHACIRA_EINVAL;
        if (cell_level < 0 || cell_level > SHACIRA_OCTREE_MAX_LEVEL) return SHACIRA_EINVAL;
        if (num_cells * (int64_t)samples_per_cell != n) return SHACIRA_EINVAL;
    }
    if (occupancy_words && (occupancy_level < 0 || occupancy_level > SHACIRA_OCTREE_MAX_LEVEL)) return SHACIRA_EINVAL;
    if (n == 0) return 1;
    if (faces && (num_triangles < 1 || !triangles || !cdf)) return SHACIRA_EINVAL;
    if (mode == SHACIRA_MESH_SAMPLE_CELLS && !corners) return SHACIRA_EINVAL;
    a.mode = mode;
    a.key0 = (uint32_t)seed;
    a.key1 = (uint32_t)(seed >> 32);
    a.segment = segment;
    a.n = n;
    a.index_base = index_base;
    a.words = words;
    a.num_triangles = faces ? num_triangles : 0;
    a.triangles = triangles;
    a.cdf = cdf;
    a.sigma = sigma;
    a.samples_per_cell = samples_per_cell;
    a.cell_level = cell_level;
    a.corners = corners;
    a.occupancy = occupancy_words;
    a.occupancy_level = occupancy_level;
    return 0;
}

int shacira_mesh_sample_count(int mode, int64_t n, int64_t index_base, uint64_t seed, uint32_t segment, const uint32_t *words,
                              int64_t num_triangles, const float *triangles, const uint32_t *cdf, float sigma,
                              int64_t num_cells, const int16_t *corners, int samples_per_cell, int cell_level,
                              const uint32_t *occupancy_words, int occupancy_level, int32_t *block_counts, void *stream) {
    MeshSampleArgs a;
    const int rc = mesh_sample_args(mode, n, index_base, seed, segment, words, num_triangles, triangles, cdf, sigma, num_cells,
                                    corners, samples_per_cell, cell_level, occupancy_words, occupancy_level, a);
    if (rc) return rc < 0 ? rc : 0;
    if (!occupancy_words || !block_counts) return SHACIRA_EINVAL;
    return (int)mesh_sample_count_dispatch(a, block_counts, (hipStream_t)stream);
}

int shacira_mesh_sample(int mode, int64_t n, int64_t index_base, uint64_t seed, uint32_t segment, const uint32_t *words,
                        int64_t num_triangles, const float *triangles, const uint32_t *cdf, float sigma, int64_t num_cells,
                        const int16_t *corners, int samples_per_cell, int cell_level, const uint32_t *occupancy_words,
                        int occupancy_level, const int64_t *block_offsets, float *points, float *normals, int32_t *face_idx,
                        int64_t *source_idx, void *stream) {
    MeshSampleArgs a;
    const int rc = mesh_sample_args(mode, n, index_base, seed, segment, words, num_triangles, triangles, cdf, sigma, num_cells,
                                    corners, samples_per_cell, cell_level, occupancy_words, occupancy_level, a);
    if (rc) return rc < 0 ? rc : 0;
    if (!points || (block_offsets == nullptr) != (occupancy_words == nullptr)) return SHACIRA_EINVAL;
    return (int)mesh_sample_write_dispatch(a, block_offsets, points, normals, face_idx, source_idx, (hipStream_t)stream);
}

// ---- structural similarity -------------------------------------------------------------------------------------------------
static bool ssim_args_ok(int64_t height, int64_t width, int pixel_stride, int channels) {
    if (height < SHACIRA_SSIM_WINDOW || width < SHACIRA_SSIM_WINDOW || channels < 1 || channels > pixel_stride) return false;
    if (pixel_stride > 65535) return false;                                  // the channel is a grid dimension
    if (height > INT64_MAX / width / pixel_stride / 16) return false;         // byte offsets and the planes stay inside int64
    return ssim_tiles(height, width) <= INT32_MAX;
}

size_t shacira_ssim_workspace_bytes(int64_t height, int64_t width, int channels, int backward) {
    if (!ssim_args_ok(height, width, channels, channels)) return 0;
    return ssim_workspace(height, width, channels, backward != 0);
}

int shacira_ssim_forward(int64_t height, int64_t width, int pixel_stride, int channels, const float *x, const float *y,
                         float data_range, double *value, float *map, void *workspace, size_t workspace_bytes,
                         void *stream) {
    if (!ssim_args_ok(height, width, pixel_stride, channels) || !(data_range > 0.f) || std::isinf(data_range))
        return SHACIRA_EINVAL;
    if (!x || !y || !value) return SHACIRA_EINVAL;
    if (!workspace || workspace_bytes < ssim_workspace(height, width, channels, false)) return SHACIRA_EWORKSPACE;
    return (int)ssim_forward_dispatch(height, width, pixel_stride, channels, x, y, data_range, value, map, workspace,
                                      (hipStream_t)stream);
}

int shacira_ssim_backward(int64_t height, int64_t width, int pixel_stride, int channels, const float *x, const float *y,
                          float data_range, const float *grad, float *grad_x, void *workspace, size_t workspace_bytes,
                          void *stream) {
    if (!ssim_args_ok(height, width, pixel_stride, channels) || !(data_range > 0.f) || std::isinf(data_range))
        return SHACIRA_EINVAL;
    if (!x || !y || !grad || !grad_x) return SHACIRA_EINVAL;
    if (!workspace || workspace_bytes < ssim_workspace(height, width, channels, true)) return SHACIRA_EWORKSPACE;
    return (int)ssim_backward_dispatch(height, width, pixel_stride, channels, x, y, data_range, grad, grad_x, workspace,
                                       (hipStream_t)stream);
}

// ---- ray generation -------------------------------------------------------------------------------------------------------------
int shacira_raygen_record_floats(void) { return SHACIRA_RAYGEN_RECORD_FLOATS; }

int shacira_raygen(const float *cams, int num_views, int width, int height, const int32_t *view_idx, const int32_t *pixel_idx,
                   const float *jitter, int64_t n, const uint8_t *images, int channels, int bg_mode, float *origins, float *dirs,
                   float *rgb, uint8_t *mask, void *stream) {
    if (num_views <= 0 || width <= 0 || height <= 0 || n < 0) return SHACIRA_EINVAL;
    if ((int64_t)width * height > INT32_MAX) return SHACIRA_EINVAL;          // pixel indices are int32
    if (images && channels != 3 && channels != 4) return SHACIRA_EINVAL;
    if (bg_mode != SHACIRA_RAYGEN_BG_WHITE && bg_mode != SHACIRA_RAYGEN_BG_BLACK) return SHACIRA_EINVAL;
    if ((view_idx == nullptr) != (pixel_idx == nullptr)) return SHACIRA_EINVAL;
    if (!view_idx && n > (int64_t)num_views * ((int64_t)width * height)) return SHACIRA_EINVAL;
    if (n == 0) return 0;                       // an empty batch may come with NULL operands
    if (!cams || !origins || !dirs || (images && (!rgb || !mask))) return SHACIRA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(cams) & 15u) != 0 || (reinterpret_cast<uintptr_t>(jitter) & 7u) != 0) return SHACIRA_EINVAL;
    return (int)raygen_dispatch(cams, num_views, width, height, view_idx, pixel_idx, jitter, n, images, channels,
                                bg_mode == SHACIRA_RAYGEN_BG_BLACK, origins, dirs, rgb, mask, (hipStream_t)stream);
}

int shacira_raygen_sums(const float *cams, int num_views, int width, int height, const int32_t *view_idx,
                        const int32_t *pixel_idx, const float *jitter, int64_t n, const uint16_t *sums, int channels, int mip,
                        int bg_mode, float *origins, float *dirs, float *rgb, uint8_t *mask, void *stream) {
    if (num_views <= 0 || width <= 0 || height <= 0 || n < 0) return SHACIRA_EINVAL;
    if ((int64_t)width * height > INT32_MAX) return SHACIRA_EINVAL;          // pixel indices are int32
    if (mip < 1 || mip > SHACIRA_IMAGE_MIP_MAX) return SHACIRA_EINVAL;
    if (sums && channels != 3 && channels != 4) return SHACIRA_EINVAL;
    if (bg_mode != SHACIRA_RAYGEN_BG_WHITE && bg_mode != SHACIRA_RAYGEN_BG_BLACK) return SHACIRA_EINVAL;
    if ((view_idx == nullptr) != (pixel_idx == nullptr)) return SHACIRA_EINVAL;
    if (!view_idx && n > (int64_t)num_views * ((int64_t)width * height)) return SHACIRA_EINVAL;
    if (n == 0) return 0;                       // an empty batch may come with NULL operands
    if (!cams || !origins || !dirs || (sums && (!rgb || !mask))) return SHACIRA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(cams) & 15u) != 0 || (reinterpret_cast<uintptr_t>(jitter) & 7u) != 0) return SHACIRA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(sums) & 1u) != 0) return SHACIRA_EINVAL;
    return (int)raygen_sums_dispatch(cams, num_views, width, height, view_idx, pixel_idx, jitter, n, sums, channels, mip,
                                     bg_mode == SHACIRA_RAYGEN_BG_BLACK, origins, dirs, rgb, mask, (hipStream_t)stream);
}

// ---- mip levels of uint8 images ------------------------------------------------------------------------------------------------
int shacira_image_mip(const uint8_t *images, int64_t num_views, int64_t height, int64_t width, int channels, int mip,
                      uint16_t *sums, void *stream) {
    if (mip < 1 || mip > SHACIRA_IMAGE_MIP_MAX || channels < 1 || channels > 4) return SHACIRA_EINVAL;
    if (num_views <= 0 || height <= 0 || width <= 0) return SHACIRA_EINVAL;
    const int64_t f = (int64_t)1 << mip;
    if (height % f != 0 || width % f != 0) return SHACIRA_EINVAL;
    // (H >> mip) * (W >> mip) < 2^31: a level's pixel indices are int32 (shacira_raygen_sums); no overflow, each factor < 2^63
    if ((height >> mip) > INT32_MAX / (width >> mip)) return SHACIRA_EINVAL;
    // every byte offset stays inside int64
    if (num_views > INT64_MAX / 8 / height / width) return SHACIRA_EINVAL;
    if (!images || !sums || (reinterpret_cast<uintptr_t>(sums) & 1u) != 0) return SHACIRA_EINVAL;
    return (int)image_mip_dispatch(images, num_views, height, width, channels, mip, sums, (hipStream_t)stream);
}

// ---- structured point clouds ----------------------------------------------------------------------------------------------------
// the operands the depth entries share; 0, or SHACIRA_EINVAL. With colours: the images and their form are checked too
static int depth_args(const float *cams, int num_views, int width, int height, const float *depth, bool colours,
                      const void *images, int channels, int mip, int bg_mode, DepthArgs &a) {
    if (num_views < 0 || width <= 0 || height <= 0) return SHACIRA_EINVAL;
    if ((int64_t)width * height > INT32_MAX) return SHACIRA_EINVAL;          // pixel indices are int32
    // workgroups of 256 pixels are a grid dimension
    if (num_views > 0 && (int64_t)width * height > ((int64_t)INT32_MAX * 256) / num_views) return SHACIRA_EINVAL;
    if (colours) {
        if (mip < 0 || mip > SHACIRA_IMAGE_MIP_MAX || (channels != 3 && channels != 4)) return SHACIRA_EINVAL;
        if (bg_mode != SHACIRA_RAYGEN_BG_WHITE && bg_mode != SHACIRA_RAYGEN_BG_BLACK) return SHACIRA_EINVAL;
    }
    if (num_views > 0) {
        if (!cams || !depth || (reinterpret_cast<uintptr_t>(cams) & 15u) != 0 || (reinterpret_cast<uintptr_t>(depth) & 3u) != 0)
            return SHACIRA_EINVAL;
        if (colours && (!images || (mip > 0 && (reinterpret_cast<uintptr_t>(images) & 1u) != 0))) return SHACIRA_EINVAL;
    }
    a = DepthArgs{cams, num_views, width, height, depth, colours ? images : nullptr, colours ? channels : 3, colours ? mip : 0,
                  colours && bg_mode == SHACIRA_RAYGEN_BG_BLACK};
    return 0;
}

static bool spc_level_ok(int level) { return level >= 1 && level <= SHACIRA_OCTREE_MAX_LEVEL; }
static bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

size_t shacira_spc_num_words(int level) {
    if (!spc_level_ok(level)) return 0;
    const size_t cells = (size_t)1 << (3 * level);
    return cells < 32 ? 1 : cells / 32;
}

int shacira_depth_bounds(const float *cams, int num_views, int width, int height, const float *depth, float *bounds,
                         int64_t *count, void *stream) {
    DepthArgs a;
    const int rc = depth_args(cams, num_views, width, height, depth, false, nullptr, 0, 0, 0, a);
    if (rc != 0) return rc;
    if (num_views == 0) return 0;
    if (!bounds || !count || !aligned4(bounds) || (reinterpret_cast<uintptr_t>(count) & 7u) != 0) return SHACIRA_EINVAL;
    return (int)depth_bounds_dispatch(a, bounds, count, (hipStream_t)stream);
}

int shacira_depth_points_count(const float *cams, int num_views, int width, int height, const float *depth,
                               int32_t *block_counts, void *stream) {
    DepthArgs a;
    const int rc = depth_args(cams, num_views, width, height, depth, false, nullptr, 0, 0, 0, a);
    if (rc != 0) return rc;
    if (num_views == 0) return 0;
    if (!block_counts) return SHACIRA_EINVAL;
    return (int)depth_points_dispatch(true, a, block_counts, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int shacira_depth_points_emit(const float *cams, int num_views, int width, int height, const float *depth, const void *images,
                              int channels, int mip, int bg_mode, const int64_t *block_offsets, float *points, uint8_t *rgb,
                              void *stream) {
    DepthArgs a;
    const int rc = depth_args(cams, num_views, width, height, depth, rgb != nullptr, images, channels, mip, bg_mode, a);
    if (rc != 0) return rc;
    if (num_views == 0) return 0;
    if (!block_offsets || !points || !aligned4(points)) return SHACIRA_EINVAL;
    return (int)depth_points_dispatch(false, a, nullptr, block_offsets, points, rgb, (hipStream_t)stream);
}

int shacira_spc_mark_points(int64_t n, const float *points, int level, uint32_t *words, void *stream) {
    if (n < 0 || !spc_level_ok(level)) return SHACIRA_EINVAL;
    if (n == 0) return 0;
    if (!points || !words || !aligned4(points) || !aligned4(words)) return SHACIRA_EINVAL;
    return (int)spc_mark_points_dispatch(n, points, level, words, (hipStream_t)stream);
}

int shacira_spc_mark_depth(const float *cams, int num_views, int width, int height, const float *depth, int level,
                           uint32_t *words, void *stream) {
    DepthArgs a;
    const int rc = depth_args(cams, num_views, width, height, depth, false, nullptr, 0, 0, 0, a);
    if (rc != 0) return rc;
    if (!spc_level_ok(level)) return SHACIRA_EINVAL;
    if (num_views == 0) return 0;
    if (!words || !aligned4(words)) return SHACIRA_EINVAL;
    return (int)spc_mark_depth_dispatch(a, level, words, (hipStream_t)stream);
}

int shacira_spc_rank(int level, const uint32_t *words, int32_t *rank, void *stream) {
    if (!spc_level_ok(level)) return SHACIRA_EINVAL;
    if (!words || !rank || !aligned4(words) || !aligned4(rank)) return SHACIRA_EINVAL;
    return (int)spc_popcount_dispatch((int64_t)shacira_spc_num_words(level), words, rank, (hipStream_t)stream);
}

int shacira_spc_accumulate_points(int64_t n, const float *points, const uint8_t *rgb, int level, const uint32_t *words,
                                  const int32_t *rank, int64_t cells, uint64_t *sums, void *stream) {
    if (n < 0 || cells < 0 || !spc_level_ok(level)) return SHACIRA_EINVAL;
    if (n == 0 || cells == 0) return 0;
    if (!points || !rgb || !words || !rank || !sums) return SHACIRA_EINVAL;
    if (!aligned4(points) || !aligned4(words) || !aligned4(rank) || (reinterpret_cast<uintptr_t>(sums) & 7u) != 0)
        return SHACIRA_EINVAL;
    return (int)spc_accumulate_points_dispatch(n, points, rgb, level, words, rank, cells, sums, (hipStream_t)stream);
}

int shacira_spc_accumulate_depth(const float *cams, int num_views, int width, int height, const float *depth, const void *images,
                                 int channels, int mip, int bg_mode, int level, const uint32_t *words, const int32_t *rank,
                                 int64_t cells, uint64_t *sums, void *stream) {
    DepthArgs a;
    const int rc = depth_args(cams, num_views, width, height, depth, true, images, channels, mip, bg_mode, a);
    if (rc != 0) return rc;
    if (cells < 0 || !spc_level_ok(level)) return SHACIRA_EINVAL;
    if (num_views == 0 || cells == 0) return 0;
    if (!words || !rank || !sums) return SHACIRA_EINVAL;
    if (!aligned4(words) || !aligned4(rank) || (reinterpret_cast<uintptr_t>(sums) & 7u) != 0) return SHACIRA_EINVAL;
    return (int)spc_accumulate_depth_dispatch(a, level, words, rank, cells, sums, (hipStream_t)stream);
}

int shacira_spc_resolve(int64_t cells, const uint64_t *sums, uint8_t *colors, void *stream) {
    if (cells < 0) return SHACIRA_EINVAL;
    if (cells == 0) return 0;
    if (!sums || !colors || (reinterpret_cast<uintptr_t>(sums) & 7u) != 0 || !aligned4(colors)) return SHACIRA_EINVAL;
    return (int)spc_resolve_dispatch(cells, sums, colors, (hipStream_t)stream);
}

int shacira_spc_first_hit(int64_t num_rays, const float *origins, const float *dirs, int level, const uint32_t *words,
                          const int32_t *rank, const uint8_t *colors, float *depth, uint8_t *hit, int32_t *pidx, float *rgb,
                          void *stream) {
    if (num_rays < 0 || num_rays > INT32_MAX || !spc_level_ok(level)) return SHACIRA_EINVAL;
    if (num_rays == 0) return 0;
    if (!origins || !dirs || !words || !depth || !hit || !pidx || (colors && (!rank || !rgb))) return SHACIRA_EINVAL;
    if (!aligned4(origins) || !aligned4(dirs) || !aligned4(words) || !aligned4(rank) || !aligned4(colors) || !aligned4(depth) ||
        !aligned4(pidx) || !aligned4(rgb))
        return SHACIRA_EINVAL;
    return (int)spc_first_hit_dispatch(num_rays, origins, dirs, level, words, rank, colors, depth, hit, pidx, rgb,
                                       (hipStream_t)stream);
}

// ---- pixel batches and the pixel loss ------------------------------------------------------------------------------------------
// the operands the three calls share: the image's size, the index form and the range
static bool pixel_args_ok(int64_t height, int64_t width, const void *pixel_idx, int idx_bits, int64_t start, int64_t n) {
    if (height <= 0 || width <= 0 || height > INT32_MAX || width > INT32_MAX || n < 0) return false;
    if (pixel_idx) return idx_bits == 32 || idx_bits == 64;
    return start >= 0 && n <= height * width && start <= height * width - n;      // the range form
}

int shacira_pixel_batch(const uint8_t *image, int64_t height, int64_t width, const void *pixel_idx, int idx_bits, int64_t start,
                        int64_t n, float *coords, float *rgb, void *stream) {
    if (!pixel_args_ok(height, width, pixel_idx, idx_bits, start, n)) return SHACIRA_EINVAL;
    if (n == 0) return 0;                       // an empty batch may come with NULL operands
    if (!image || (!coords && !rgb)) return SHACIRA_EINVAL;
    return (int)pixel_batch_dispatch(image, height, width, pixel_idx, idx_bits, start, n, coords, rgb, (hipStream_t)stream);
}

size_t shacira_pixel_loss_workspace_bytes(int64_t n) { return pixel_loss_workspace(n); }

static bool pixel_pred_ok(int64_t n, int64_t pred_stride) {       // byte offsets stay inside int64
    return pred_stride >= 3 && pred_stride <= INT64_MAX / 16 / (n > 0 ? n : 1);
}

int shacira_pixel_loss_forward(const float *pred, int64_t pred_stride, const uint8_t *image, int64_t height, int64_t width,
                               const void *pixel_idx, int idx_bits, int64_t start, int64_t n, uint8_t *out_image, double *stats,
                               void *workspace, size_t workspace_bytes, void *stream) {
    if (!pixel_args_ok(height, width, pixel_idx, idx_bits, start, n) || !pixel_pred_ok(n, pred_stride)) return SHACIRA_EINVAL;
    if (n == 0) return 0;
    if (!pred || !image || !stats) return SHACIRA_EINVAL;
    if (!workspace || workspace_bytes < pixel_loss_workspace(n)) return SHACIRA_EINVAL;
    return (int)pixel_loss_forward_dispatch(pred, pred_stride, image, height, width, pixel_idx, idx_bits, start, n, out_image,
                                            stats, workspace, (hipStream_t)stream);
}

int shacira_pixel_loss_backward(const float *pred, int64_t pred_stride, const uint8_t *image, int64_t height, int64_t width,
                                const void *pixel_idx, int idx_bits, int64_t start, int64_t n, const float *grad,
                                float *grad_pred, void *stream) {
    if (!pixel_args_ok(height, width, pixel_idx, idx_bits, start, n) || !pixel_pred_ok(n, pred_stride)) return SHACIRA_EINVAL;
    if (n == 0) return 0;
    if (!pred || !image || !grad || !grad_pred) return SHACIRA_EINVAL;
    return (int)pixel_loss_backward_dispatch(pred, pred_stride, image, height, width, pixel_idx, idx_bits, start, n, grad,
                                             grad_pred, (hipStream_t)stream);
}

// ---- positional-encoding rows ----------------------------------------------------------------------------------------------
// the shape shared by the three calls; `width` = P + E. Row strides are checked by the callers
static bool posenc_shape_ok(int64_t n, int d, int num_bands, int64_t prefix_width, int64_t *width) {
    if (n < 0 || prefix_width < 0 || prefix_width > SHACIRA_POSENC_MAX_PREFIX) return false;
    if (d < 1 || d > SHACIRA_POSENC_MAX_DIM || num_bands < 1 || num_bands > SHACIRA_POSENC_MAX_BANDS) return false;
    *width = prefix_width + 2 * (int64_t)d * num_bands;
    return true;
}

static bool posenc_rows_fit(int64_t n, int64_t stride) {       // byte offsets stay inside int64
    return stride <= INT64_MAX / 16 / (n > 0 ? n : 1);
}

int shacira_posenc_forward(int64_t n, int d, int num_bands, int include_input, int64_t prefix_width, const float *coords,
                           int64_t coords_stride, const float *prefix, int64_t prefix_stride, const float *bands, float *out,
                           int64_t out_stride, void *stream) {
    int64_t width;
    if (!posenc_shape_ok(n, d, num_bands, prefix_width, &width)) return SHACIRA_EINVAL;
    const int I = include_input ? d : 0;
    width += I;
    if (n == 0) return 0;                       // an empty batch may come with NULL operands
    if (!coords || !bands || !out || (prefix_width > 0 && !prefix)) return SHACIRA_EINVAL;
    if (out_stride < width || coords_stride < d || (prefix_width > 0 && prefix_stride < prefix_width)) return SHACIRA_EINVAL;
    if (!posenc_rows_fit(n, out_stride) || !posenc_rows_fit(n, coords_stride) ||
        (prefix_width > 0 && !posenc_rows_fit(n, prefix_stride)))
        return SHACIRA_EINVAL;
    return (int)posenc_forward_dispatch(n, d, num_bands, I, (int)prefix_width, coords, coords_stride, prefix,
                                        prefix_width > 0 ? prefix_stride : 0, bands, out, out_stride, (hipStream_t)stream);
}

int shacira_posenc_backward(int64_t n, int d, int num_bands, int include_input, int64_t prefix_width, const float *row,
                            int64_t row_stride, const float *grad_out, int64_t grad_stride, const float *bands,
                            float *grad_coords, void *stream) {
    int64_t width;
    if (!posenc_shape_ok(n, d, num_bands, prefix_width, &width)) return SHACIRA_EINVAL;
    const int I = include_input ? d : 0;
    width += I;
    if (n == 0) return 0;
    if (!row || !grad_out || !bands || !grad_coords) return SHACIRA_EINVAL;
    if (row_stride < width || grad_stride < width) return SHACIRA_EINVAL;
    if (!posenc_rows_fit(n, row_stride) || !posenc_rows_fit(n, grad_stride)) return SHACIRA_EINVAL;
    return (int)posenc_backward_dispatch(n, d, num_bands, I, (int)prefix_width, row, row_stride, grad_out, grad_stride, bands,
                                         grad_coords, (hipStream_t)stream);
}

int shacira_posenc_backward2(int64_t n, int d, int num_bands, int include_input, int64_t prefix_width, const float *gg,
                             const float *row, int64_t row_stride, const float *grad_out, int64_t grad_stride,
                             const float *bands, float *grad_row, float *grad_grad_out, void *stream) {
    int64_t width;
    if (!posenc_shape_ok(n, d, num_bands, prefix_width, &width)) return SHACIRA_EINVAL;
    const int I = include_input ? d : 0;
    width += I;
    if (n == 0) return 0;
    if (!gg || !row || !grad_out || !bands || !grad_row || !grad_grad_out) return SHACIRA_EINVAL;
    if (row_stride < width || grad_stride < width) return SHACIRA_EINVAL;
    if (!posenc_rows_fit(n, row_stride) || !posenc_rows_fit(n, grad_stride)) return SHACIRA_EINVAL;
    return (int)posenc_backward2_dispatch(n, d, num_bands, I, (int)prefix_width, gg, row, row_stride, grad_out, grad_stride,
                                          bands, grad_row, grad_grad_out, (hipStream_t)stream);
}

// ---- sphere tracing over ray packs ---------------------------------------------------------------------------------------
static bool trace_counts_ok(int64_t num_packs, int64_t num_nugs) {
    return num_packs >= 0 && num_nugs >= 0 && num_packs <= INT32_MAX && num_nugs <= INT32_MAX && num_packs <= num_nugs;
}

int shacira_find_depth_bound(int64_t num_packs, int64_t num_nugs, const float *query, const int32_t *curr_idxes,
                             const int32_t *pack_end, const float *depth, int32_t *out, void *stream) {
    if (!trace_counts_ok(num_packs, num_nugs)) return SHACIRA_EINVAL;
    if (num_packs == 0) return 0;
    if (!query || !curr_idxes || !pack_end || !depth || !out) return SHACIRA_EINVAL;
    return (int)find_depth_bound_launch(num_packs, num_nugs, query, curr_idxes, pack_end, depth, out, (hipStream_t)stream);
}

int shacira_sphere_trace_step(int64_t num_packs, int64_t num_nugs, int64_t num_active, int first_iteration,
                              const int32_t *active_in, const float *sdf, const float *origins, const float *dirs,
                              const float *depth, const int32_t *pack_end, const int32_t *pidx, float step_size,
                              float min_dis, float dist_max, float *t, float *dist, float *dist_prev, int32_t *curr,
                              float *x, uint8_t *active, uint8_t *hit, int32_t *active_out, float *coords_out,
                              int32_t *pidx_out, int32_t *count_out, int32_t *count_next, void *stream) {
    if (!trace_counts_ok(num_packs, num_nugs)) return SHACIRA_EINVAL;
    if (num_active < 0 || num_active > num_packs) return SHACIRA_EINVAL;
    if (num_active == 0) return 0;
    if (!active_in || !sdf || !origins || !dirs || !depth || !pack_end || !t || !dist || !dist_prev || !curr || !x ||
        !active || !hit || !active_out || !coords_out || !count_out || !count_next || count_out == count_next)
        return SHACIRA_EINVAL;
    if (pidx && !pidx_out) return SHACIRA_EINVAL;
    return (int)sphere_trace_step_launch(num_packs, num_nugs, num_active, first_iteration != 0, active_in, sdf, origins,
                                         dirs, depth, pack_end, pidx, step_size, min_dis, dist_max, t, dist, dist_prev,
                                         curr, x, active, hit, active_out, coords_out, pidx_out, count_out, count_next,
                                         (hipStream_t)stream);
}

// ---- view shading ---------------------------------------------------------------------------------------------------------------
int shacira_shade_view(int64_t n, int mode, float *normal, const float *dirs, const uint8_t *hit, const float *mm_host,
                       const uint8_t *tex, int mh, int mw, int mc, float *rgb, float *uv_out, uint8_t *rgb8_out, void *stream) {
    if (n < 0) return SHACIRA_EINVAL;
    if (mode != SHACIRA_SHADE_RB && mode != SHACIRA_SHADE_NORMAL && mode != SHACIRA_SHADE_MATCAP) return SHACIRA_EINVAL;
    if (mode != SHACIRA_SHADE_MATCAP && uv_out) return SHACIRA_EINVAL;
    if (mode == SHACIRA_SHADE_MATCAP && tex &&
        ((mc != 3 && mc != 4) || mh < 2 || mw < 2 || mh > SHACIRA_SHADE_MAX_TEX || mw > SHACIRA_SHADE_MAX_TEX))
        return SHACIRA_EINVAL;
    if (n == 0) return 0;                       // an empty view may come with NULL operands
    if (mode == SHACIRA_SHADE_MATCAP && !tex) {                 // the coordinates-only form
        if (!uv_out || rgb || rgb8_out || hit) return SHACIRA_EINVAL;
    } else if (!rgb) {
        return SHACIRA_EINVAL;
    }
    if (mode != SHACIRA_SHADE_RB && !normal) return SHACIRA_EINVAL;
    if (mode == SHACIRA_SHADE_MATCAP && !dirs) return SHACIRA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(uv_out) & 7u) != 0) return SHACIRA_EINVAL;
    if (mode != SHACIRA_SHADE_MATCAP) tex = nullptr;
    return (int)shade_view_dispatch(n, mode, normal, dirs, hit, mode == SHACIRA_SHADE_MATCAP ? mm_host : nullptr, tex, mh, mw, mc,
                                    rgb, uv_out, rgb8_out, (hipStream_t)stream);
}

int shacira_shadow_rays(int64_t n, const float *origins, const float *dirs, const float *light_host, float min_y, uint64_t seed,
                        float *depth, float *xyz, float *normal, uint8_t *hit, float *so, float *sd, uint8_t *light_hit,
                        uint8_t *plane_hit, void *stream) {
    if (n < 0) return SHACIRA_EINVAL;
    if (n == 0) return 0;
    if (!origins || !dirs || !light_host || !depth || !xyz || !normal || !hit || !so || !sd || !light_hit || !plane_hit)
        return SHACIRA_EINVAL;
    return (int)shadow_rays_dispatch(n, origins, dirs, light_host, min_y, seed, depth, xyz, normal, hit, so, sd, light_hit,
                                     plane_hit, (hipStream_t)stream);
}

// each side below 2^30: the kernels' reflect period 2 n and the taps' y +- 8 stay inside an int
static bool shadow_apply_sizes_ok(int64_t height, int64_t width) {
    const int64_t side = (int64_t)1 << 30;
    return height >= 1 && width >= 1 && height < side && width < side && height * width <= INT32_MAX;
}

static bool bytes_overlap(const void *a, const void *b, int64_t n) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb ? pb - pa < (uintptr_t)n : pa - pb < (uintptr_t)n;
}

size_t shacira_shadow_apply_workspace_bytes(int64_t height, int64_t width) {
    return shadow_apply_sizes_ok(height, width) ? (size_t)(height * width) * sizeof(float) : 0;
}

int shacira_shadow_apply(int64_t height, int64_t width, int channels, const uint8_t *occluded, const uint8_t *light_hit,
                         uint8_t *shadow_out, float *rgb, void *workspace, size_t workspace_bytes, void *stream) {
    if (!shadow_apply_sizes_ok(height, width) || (channels != 3 && channels != 4)) return SHACIRA_EINVAL;
    if (!occluded || !light_hit || !shadow_out || !rgb) return SHACIRA_EINVAL;
    if (bytes_overlap(shadow_out, occluded, height * width) || bytes_overlap(shadow_out, light_hit, height * width))
        return SHACIRA_EINVAL;
    if (channels == 4 && (reinterpret_cast<uintptr_t>(rgb) & 15u) != 0) return SHACIRA_EINVAL;
    if (!workspace || workspace_bytes < shacira_shadow_apply_workspace_bytes(height, width)) return SHACIRA_EWORKSPACE;
    return (int)shadow_apply_dispatch(height, width, channels, occluded, light_hit, shadow_out, rgb, workspace,
                                      (hipStream_t)stream);
}

int shacira_sdf_slice_colors(int64_t n, const float *d, float *vis, void *stream) {
    if (n < 0) return SHACIRA_EINVAL;
    if (n == 0) return 0;
    if (!d || !vis) return SHACIRA_EINVAL;
    return (int)sdf_slice_colors_dispatch(n, d, vis, (hipStream_t)stream);
}

// ---- affine latent decoders: plain, SGA, SGA with the temperature on the device, per-level ---------------------------------
static int levels_args_ok(int num_levels, const int64_t *row_offsets_host, int64_t num_rows, int latent_dim,
                          int feature_dim) {
    if (num_levels < 1 || num_levels > SHACIRA_MAX_LODS || !row_offsets_host) return SHACIRA_EINVAL;
    if (num_rows < 0 || latent_dim < 1 || feature_dim < 1) return SHACIRA_EINVAL;
    if (!latent_decode_supported(latent_dim, feature_dim)) return SHACIRA_EDTYPE;
    int64_t prev = 0;
    for (int l = 0; l <= num_levels; ++l) {
        const int64_t o = row_offsets_host[l];
        if (o < 0 || o > num_rows) return SHACIRA_EINVAL;
        if (l < num_levels && o < prev) return SHACIRA_EINVAL;   // level starts ascend; the LAST boundary may fall short
        prev = o;
    }
    return 0;
}

enum DecodeKind { DECODE_ROUND, DECODE_SGA, DECODE_SGA_TDEV, DECODE_LEVELS };

// All eight entry points below; everything but DECODE_LEVELS runs as the one level {0, num_rows} (no offsets). The order of
// the checks is each entry point's own (it decides which error code a call with several faults gets).
static int latent_decode_call(bool bwd, DecodeKind kind, int num_levels, const int64_t *row_offsets_host, int64_t num_rows,
                              int latent_dim, int feature_dim, const float *latent, const float *uniforms, float temperature,
                              const float *temperature_dev, int diff_sampling, const float *div, const float *matrix,
                              const float *colscale, const float *shift, float clamp_weights, float *decoded,
                              const float *grad_decoded, float *grad_latent, float *grad_matrix, float *grad_colscale,
                              float *grad_shift, void *workspace, size_t workspace_bytes, void *stream) {
    if (kind == DECODE_LEVELS) {
        if (int rc = levels_args_ok(num_levels, row_offsets_host, num_rows, latent_dim, feature_dim)) return rc;
        if (uniforms && !(temperature > 0.0f)) return SHACIRA_EINVAL;
    } else {
        if (num_rows < 0 || latent_dim < 1 || feature_dim < 1) return SHACIRA_EINVAL;
        if (kind == DECODE_SGA && !(temperature > 0.0f)) return SHACIRA_EINVAL;
        if (kind == DECODE_SGA_TDEV && !temperature_dev) return SHACIRA_EINVAL;
        if (!latent_decode_supported(latent_dim, feature_dim)) return SHACIRA_EDTYPE;
        num_levels = 1;
        row_offsets_host = nullptr;
    }
    if (bwd && (!workspace || workspace_bytes < latent_workspace_bytes())) return SHACIRA_EWORKSPACE;
    if (!bwd && num_rows == 0) return 0;
    const bool sga = kind == DECODE_SGA || kind == DECODE_SGA_TDEV;
    if (num_rows > 0 && (!latent || !div || !matrix || (bwd ? !grad_decoded : !decoded) || (sga && !uniforms)))
        return SHACIRA_EINVAL;
    // rows no level owns (before the first level, after the last boundary) decode to 0 and get no gradient
    float *unowned = bwd ? grad_latent : decoded;
    if (kind == DECODE_LEVELS && unowned && num_rows > 0) {
        const size_t n = (size_t)num_rows * (bwd ? latent_dim : feature_dim) * sizeof(float);
        hipError_t e = hipMemsetAsync(unowned, 0, n, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    DecodeArgs a{};
    a.latent = latent; a.div = div; a.matrix = matrix; a.colscale = colscale; a.shift = shift;
    a.clampw = clamp_weights; a.decoded = decoded; a.grad_decoded = grad_decoded; a.grad_latent = grad_latent;
    a.grad_matrix = grad_matrix; a.grad_colscale = grad_colscale; a.grad_shift = grad_shift;
    a.partials = static_cast<double *>(workspace); a.rows = num_rows;
    a.uniforms = uniforms; a.temperature = temperature; a.temperature_dev = temperature_dev; a.diff_sampling = diff_sampling;
    return (int)latent_decode_dispatch(bwd, latent_dim, feature_dim, num_levels, row_offsets_host, a, (hipStream_t)stream);
}

int shacira_latent_decode_forward(int64_t num_rows, int latent_dim, int feature_dim, const float *latent,
                                  const float *div, const float *matrix, const float *colscale, const float *shift,
                                  float clamp_weights, float *decoded, void *stream) {
    return latent_decode_call(false, DECODE_ROUND, 1, nullptr, num_rows, latent_dim, feature_dim, latent, nullptr, 0.0f,
                              nullptr, 0, div, matrix, colscale, shift, clamp_weights, decoded, nullptr, nullptr, nullptr,
                              nullptr, nullptr, nullptr, 0, stream);
}

size_t shacira_latent_decode_backward_workspace_bytes(int64_t, int, int) { return latent_workspace_bytes(); }

int shacira_latent_decode_backward(int64_t num_rows, int latent_dim, int feature_dim, const float *latent,
                                   const float *div, const float *matrix, const float *colscale, const float *shift,
                                   float clamp_weights, const float *grad_decoded, float *grad_latent,
                                   float *grad_matrix, float *grad_colscale, float *grad_shift, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    return latent_decode_call(true, DECODE_ROUND, 1, nullptr, num_rows, latent_dim, feature_dim, latent, nullptr, 0.0f,
                              nullptr, 0, div, matrix, colscale, shift, clamp_weights, nullptr, grad_decoded, grad_latent,
                              grad_matrix, grad_colscale, grad_shift, workspace, workspace_bytes, stream);
}

int shacira_latent_decode_sga_forward(int64_t num_rows, int latent_dim, int feature_dim, const float *latent,
                                      const float *uniforms, float temperature, int diff_sampling, const float *div,
                                      const float *matrix, const float *colscale, const float *shift,
                                      float clamp_weights, float *decoded, void *stream) {
    return latent_decode_call(false, DECODE_SGA, 1, nullptr, num_rows, latent_dim, feature_dim, latent, uniforms,
                              temperature, nullptr, diff_sampling, div, matrix, colscale, shift, clamp_weights, decoded,
                              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, stream);
}

int shacira_latent_decode_sga_backward(int64_t num_rows, int latent_dim, int feature_dim, const float *latent,
                                       const float *uniforms, float temperature, int diff_sampling, const float *div,
                                       const float *matrix, const float *colscale, const float *shift,
                                       float clamp_weights, const float *grad_decoded, float *grad_latent,
                                       float *grad_matrix, float *grad_colscale, float *grad_shift, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    return latent_decode_call(true, DECODE_SGA, 1, nullptr, num_rows, latent_dim, feature_dim, latent, uniforms,
                              temperature, nullptr, diff_sampling, div, matrix, colscale, shift, clamp_weights, nullptr,
                              grad_decoded, grad_latent, grad_matrix, grad_colscale, grad_shift, workspace,
                              workspace_bytes, stream);
}

// The same pair with the temperature in DEVICE memory (one float, read by the kernels): a training step captured into a HIP
// graph anneals the temperature between replays (base_trainer.py:155-157 decays it every iteration) without re-capturing.
int shacira_latent_decode_sga_forward_tdev(int64_t num_rows, int latent_dim, int feature_dim, const float *latent,
                                           const float *uniforms, const float *temperature_dev, int diff_sampling,
                                           const float *div, const float *matrix, const float *colscale, const float *shift,
                                           float clamp_weights, float *decoded, void *stream) {
    return latent_decode_call(false, DECODE_SGA_TDEV, 1, nullptr, num_rows, latent_dim, feature_dim, latent, uniforms, 1.0f,
                              temperature_dev, diff_sampling, div, matrix, colscale, shift, clamp_weights, decoded, nullptr,
                              nullptr, nullptr, nullptr, nullptr, nullptr, 0, stream);
}

int shacira_latent_decode_sga_backward_tdev(int64_t num_rows, int latent_dim, int feature_dim, const float *latent,
                                            const float *uniforms, const float *temperature_dev, int diff_sampling,
                                            const float *div, const float *matrix, const float *colscale, const float *shift,
                                            float clamp_weights, const float *grad_decoded, float *grad_latent,
                                            float *grad_matrix, float *grad_colscale, float *grad_shift, void *workspace,
                                            size_t workspace_bytes, void *stream) {
    return latent_decode_call(true, DECODE_SGA_TDEV, 1, nullptr, num_rows, latent_dim, feature_dim, latent, uniforms, 1.0f,
                              temperature_dev, diff_sampling, div, matrix, colscale, shift, clamp_weights, nullptr,
                              grad_decoded, grad_latent, grad_matrix, grad_colscale, grad_shift, workspace,
                              workspace_bytes, stream);
}

int shacira_latent_decode_levels_forward(int num_levels, const int64_t *row_offsets_host, int64_t num_rows,
                                         int latent_dim, int feature_dim, const float *latent, const float *uniforms,
                                         float temperature, int diff_sampling, const float *div, const float *matrix,
                                         const float *colscale, const float *shift, float clamp_weights, float *decoded,
                                         void *stream) {
    return latent_decode_call(false, DECODE_LEVELS, num_levels, row_offsets_host, num_rows, latent_dim, feature_dim, latent,
                              uniforms, temperature, nullptr, diff_sampling, div, matrix, colscale, shift, clamp_weights,
                              decoded, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, stream);
}

int shacira_latent_decode_levels_backward(int num_levels, const int64_t *row_offsets_host, int64_t num_rows,
                                          int latent_dim, int feature_dim, const float *latent, const float *uniforms,
                                          float temperature, int diff_sampling, const float *div, const float *matrix,
                                          const float *colscale, const float *shift, float clamp_weights,
                                          const float *grad_decoded, float *grad_latent, float *grad_matrix,
                                          float *grad_colscale, float *grad_shift, void *workspace,
                                          size_t workspace_bytes, void *stream) {
    return latent_decode_call(true, DECODE_LEVELS, num_levels, row_offsets_host, num_rows, latent_dim, feature_dim, latent,
                              uniforms, temperature, nullptr, diff_sampling, div, matrix, colscale, shift, clamp_weights,
                              nullptr, grad_decoded, grad_latent, grad_matrix, grad_colscale, grad_shift, workspace,
                              workspace_bytes, stream);
}

int shacira_latent_mlp_supported(int num_layers, const int32_t *widths_host) {
    return latent_mlp_supported(num_layers, widths_host) ? 1 : 0;
}

size_t shacira_latent_mlp_backward_workspace_bytes(int num_layers, const int32_t *widths_host) {
    return latent_mlp_workspace_bytes(num_layers, widths_host);
}

static int latent_mlp_call(bool bwd, int64_t num_rows, int num_layers, const int32_t *widths_host, const float *latent,
                           const float *uniforms, float temperature, int diff_sampling, const float *div,
                           const float *params, int activation, int final_activation, float clamp_weights, float *decoded,
                           const float *grad_decoded, float *grad_latent, float *grad_params, void *workspace,
                           size_t workspace_bytes, void *stream) {
    options_snapshot();
    if (num_rows < 0 || !latent_mlp_supported(num_layers, widths_host)) return SHACIRA_EINVAL;
    if (activation < SHACIRA_ACT_NONE || activation > SHACIRA_ACT_SINE30 || final_activation < SHACIRA_ACT_NONE ||
        final_activation > SHACIRA_ACT_SINE30)
        return SHACIRA_EINVAL;
    if (!div || !params) return SHACIRA_EINVAL;
    if (num_rows > 0 && (!latent || (bwd ? !grad_decoded : !decoded))) return SHACIRA_EINVAL;
    if (uniforms && !(temperature > 0.0f)) return SHACIRA_EINVAL;
    if (bwd) {
        if (!grad_params) return SHACIRA_EINVAL;
        if (!workspace || workspace_bytes < latent_mlp_workspace_bytes(num_layers, widths_host)) return SHACIRA_EWORKSPACE;
    }
    LatentMlpArgs a{};
    a.num_layers = num_layers; a.widths = widths_host; a.latent = latent; a.uniforms = uniforms; a.div = div;
    a.params = params; a.temperature = temperature; a.diff_sampling = diff_sampling; a.act = activation;
    a.final_act = final_activation; a.clampw = clamp_weights; a.decoded = decoded; a.grad_decoded = grad_decoded;
    a.grad_latent = grad_latent; a.grad_params = grad_params; a.partials = static_cast<double *>(workspace);
    a.rows = num_rows;
    return (int)latent_mlp_dispatch(bwd, a, (hipStream_t)stream);
}

int shacira_latent_mlp_forward(int64_t num_rows, int num_layers, const int32_t *widths_host, const float *latent,
                               const float *uniforms, float temperature, int diff_sampling, const float *div,
                               const float *params, int activation, int final_activation, float clamp_weights,
                               float *decoded, void *stream) {
    return latent_mlp_call(false, num_rows, num_layers, widths_host, latent, uniforms, temperature, diff_sampling, div, params,
                           activation, final_activation, clamp_weights, decoded, nullptr, nullptr, nullptr, nullptr, 0,
                           stream);
}

int shacira_latent_mlp_backward(int64_t num_rows, int num_layers, const int32_t *widths_host, const float *latent,
                                const float *uniforms, float temperature, int diff_sampling, const float *div,
                                const float *params, int activation, int final_activation, float clamp_weights,
                                const float *grad_decoded, float *grad_latent, float *grad_params, void *workspace,
                                size_t workspace_bytes, void *stream) {
    return latent_mlp_call(true, num_rows, num_layers, widths_host, latent, uniforms, temperature, diff_sampling, div, params,
                           activation, final_activation, clamp_weights, nullptr, grad_decoded, grad_latent, grad_params,
                           workspace, workspace_bytes, stream);
}

int shacira_latent_multi_supported(int latent_dim, int feature_dim, int num_decoders) {
    return latent_multi_supported(latent_dim, feature_dim, num_decoders) ? 1 : 0;
}

static int multi_args_ok(int64_t num_rows, int latent_dim, int feature_dim, int num_decoders, float temperature) {
    if (num_rows < 0 || latent_dim < 1 || feature_dim < 1 || num_decoders < 1 || !(temperature > 0.0f)) return SHACIRA_EINVAL;
    if (!latent_multi_supported(latent_dim, feature_dim, num_decoders)) return SHACIRA_EDTYPE;
    return 0;
}

int shacira_latent_multi_decode_forward(int64_t num_rows, int latent_dim, int feature_dim, int num_decoders,
                                        const float *latent, const float *alpha, const float *uniforms,
                                        float temperature, int straight_through, int diff_sampling, const float *div,
                                        const float *scale, const float *dft, const float *shift, float clamp_weights,
                                        float *decoded, void *stream) {
    if (int rc = multi_args_ok(num_rows, latent_dim, feature_dim, num_decoders, temperature)) return rc;
    if (num_rows == 0) return 0;
    if (!latent || !alpha || !div || !scale || !decoded) return SHACIRA_EINVAL;
    MultiArgs a{};
    a.latent = latent; a.alpha = alpha; a.div = div; a.scale = scale; a.dft = dft; a.shift = shift; a.uniforms = uniforms;
    a.decoded = decoded; a.rows = num_rows; a.K = num_decoders; a.straight_through = straight_through;
    a.diff_sampling = diff_sampling; a.temperature = temperature; a.clampw = clamp_weights;
    return (int)latent_multi_dispatch(false, latent_dim, feature_dim, dft != nullptr, a, (hipStream_t)stream);
}

int shacira_latent_multi_decode_backward(int64_t num_rows, int latent_dim, int feature_dim, int num_decoders,
                                         const float *latent, const float *alpha, const float *uniforms,
                                         float temperature, int straight_through, int diff_sampling, const float *div,
                                         const float *scale, const float *dft, const float *shift, float clamp_weights,
                                         const float *grad_decoded, float *grad_latent, float *grad_alpha,
                                         float *grad_scale, float *grad_shift, void *workspace, size_t workspace_bytes,
                                         void *stream) {
    if (int rc = multi_args_ok(num_rows, latent_dim, feature_dim, num_decoders, temperature)) return rc;
    if (!workspace || workspace_bytes < latent_workspace_bytes()) return SHACIRA_EWORKSPACE;
    if (!grad_scale || (num_rows > 0 && (!latent || !alpha || !div || !scale || !grad_decoded))) return SHACIRA_EINVAL;
    MultiArgs a{};
    a.latent = latent; a.alpha = alpha; a.div = div; a.scale = scale; a.dft = dft; a.shift = shift; a.uniforms = uniforms;
    a.grad_decoded = grad_decoded; a.grad_latent = grad_latent; a.grad_alpha = grad_alpha; a.grad_scale = grad_scale;
    a.grad_shift = grad_shift; a.partials = static_cast<double *>(workspace); a.rows = num_rows; a.K = num_decoders;
    a.straight_through = straight_through; a.diff_sampling = diff_sampling; a.temperature = temperature;
    a.clampw = clamp_weights;
    return (int)latent_multi_dispatch(true, latent_dim, feature_dim, dft != nullptr, a, (hipStream_t)stream);
}

int shacira_latent_symbol_range(int64_t num_rows, int latent_dim, const float *latent, int32_t *minmax, void *stream) {
    if (num_rows < 0 || latent_dim < 1 || !minmax || (num_rows > 0 && !latent)) return SHACIRA_EINVAL;
    if (!symbols_supported(latent_dim)) return SHACIRA_EDTYPE;
    return (int)symbol_range_launch(latent, num_rows, latent_dim, minmax, (hipStream_t)stream);
}

int shacira_latent_symbol_histogram(int64_t num_rows, int latent_dim, const float *latent, const int32_t *minmax,
                                    int nbins, uint64_t *counts, void *stream) {
    if (num_rows < 0 || latent_dim < 1 || nbins < 1 || !minmax || !counts || (num_rows > 0 && !latent))
        return SHACIRA_EINVAL;
    if (!symbols_supported(latent_dim)) return SHACIRA_EDTYPE;
    return (int)symbol_histogram_launch(latent, num_rows, latent_dim, minmax, nbins, counts, (hipStream_t)stream);
}

size_t shacira_rc_encode_bound(int64_t n) { return rc_encode_bound(n < 0 ? 0 : n); }

int shacira_rc_encode(const int32_t *symbols_host, int64_t n, const uint32_t *freq_host, int num_symbols,
                      uint8_t *out_host, size_t capacity, size_t *out_len) {
    return rc_encode(symbols_host, n, freq_host, num_symbols, out_host, capacity, out_len);
}

int shacira_rc_decode(const uint8_t *in_host, size_t len, const uint32_t *freq_host, int num_symbols, int64_t n,
                      int32_t *symbols_host) {
    return rc_decode(in_host, len, freq_host, num_symbols, n, symbols_host);
}

size_t shacira_rans_encode_bound(int64_t n, int steps) {
    return rans_steps_ok(steps) ? rans_encode_bound(n < 0 ? 0 : n, steps) : 0;
}

int shacira_rans_encode(const int32_t *symbols_host, int64_t n, const uint32_t *freq_host, int num_symbols, int steps,
                        uint8_t *out_host, size_t capacity, size_t *out_len) {
    return rans_encode(symbols_host, n, freq_host, num_symbols, steps, out_host, capacity, out_len);
}

int shacira_rans_decode(const uint8_t *in_host, size_t len, const uint32_t *freq_host, int num_symbols, int64_t n,
                        int steps, int32_t *symbols_host) {
    return rans_decode(in_host, len, freq_host, num_symbols, n, steps, symbols_host);
}

int shacira_latent_rans_encode(int64_t num_rows, int latent_dim, const float *latent, const int32_t *lo_host,
                               const int32_t *nbins_host, const uint32_t *cdf, int cdf_stride, int steps,
                               uint32_t *counts, uint32_t *states, uint16_t *slots, void *stream) {
    int rc = rans_device_args_ok(num_rows, latent_dim, nbins_host, cdf_stride, steps, nullptr, nullptr, 0);
    if (rc) return rc;
    if (!lo_host) return SHACIRA_EINVAL;
    if (num_rows == 0) return 0;
    if (!latent || !cdf || !counts || !states || !slots) return SHACIRA_EINVAL;
    return (int)rans_encode_launch(latent, num_rows, latent_dim, lo_host, nbins_host, cdf, cdf_stride, steps, counts,
                                   states, slots, (hipStream_t)stream);
}

int shacira_latent_rans_pack(int64_t num_rows, int latent_dim, const int32_t *nbins_host, int steps,
                             const uint32_t *counts, const uint32_t *states, const uint16_t *slots,
                             const int64_t *block_start, const int64_t *payload_offset_host, const int64_t *words_host,
                             uint8_t *out, size_t out_bytes, void *stream) {
    if (!payload_offset_host || !words_host) return SHACIRA_EINVAL;
    int rc = rans_device_args_ok(num_rows, latent_dim, nbins_host, INT32_MAX, steps, payload_offset_host, words_host,
                                 out_bytes);
    if (rc) return rc;
    if (num_rows == 0) return 0;
    if (!counts || !states || !slots || !block_start || !out) return SHACIRA_EINVAL;
    return (int)rans_pack_launch(num_rows, latent_dim, nbins_host, steps, counts, states, slots, block_start,
                                 payload_offset_host, words_host, out, (hipStream_t)stream);
}

int shacira_latent_rans_decode(int64_t num_rows, int latent_dim, const uint8_t *container, size_t container_bytes,
                               const int32_t *lo_host, const int32_t *nbins_host, const int64_t *payload_offset_host,
                               const int64_t *words_host, const uint32_t *cdf, int cdf_stride,
                               const int64_t *block_start, int steps, float *out, int32_t *error, void *stream) {
    if (!payload_offset_host || !words_host) return SHACIRA_EINVAL;
    int rc = rans_device_args_ok(num_rows, latent_dim, nbins_host, cdf_stride, steps, payload_offset_host, words_host,
                                 container_bytes);
    if (rc) return rc;
    if (!lo_host || !error) return SHACIRA_EINVAL;
    if (num_rows == 0) return 0;
    if (!container || !cdf || !block_start || !out) return SHACIRA_EINVAL;
    return (int)rans_decode_launch(container, num_rows, latent_dim, lo_host, nbins_host, payload_offset_host, words_host,
                                   cdf, cdf_stride, block_start, steps, out, error, (hipStream_t)stream);
}

static int pack_args_ok(int64_t S, int64_t R, int C) {
    if (S < 0 || R < 0 || C < 1) return SHACIRA_EINVAL;
    if (C > 16) return SHACIRA_EDTYPE;
    return 0;
}

int shacira_pack_integrate_forward(int64_t num_samples, int64_t num_packs, int channels, const float *feats,
                                   const float *tau, const int64_t *pack_start, float *ray_feats, float *weights,
                                   void *stream) {
    if (int rc = pack_args_ok(num_samples, num_packs, channels)) return rc;
    if (num_packs == 0) return 0;
    if (!pack_start || !ray_feats || (num_samples > 0 && (!feats || !tau || !weights))) return SHACIRA_EINVAL;
    return (int)pack_integrate_launch(false, num_packs, channels, feats, tau, pack_start, ray_feats, weights, nullptr,
                                      nullptr, nullptr, nullptr, (hipStream_t)stream);
}

int shacira_pack_integrate_backward(int64_t num_samples, int64_t num_packs, int channels, const float *feats,
                                    const float *tau, const int64_t *pack_start, const float *grad_ray_feats,
                                    const float *grad_weights, float *grad_feats, float *grad_tau, void *stream) {
    if (int rc = pack_args_ok(num_samples, num_packs, channels)) return rc;
    if (num_packs == 0 || num_samples == 0) return 0;
    if (!pack_start || !feats || !tau || !grad_ray_feats || !grad_feats || !grad_tau) return SHACIRA_EINVAL;
    return (int)pack_integrate_launch(true, num_packs, channels, feats, tau, pack_start, nullptr, nullptr,
                                      grad_ray_feats, grad_weights, grad_feats, grad_tau, (hipStream_t)stream);
}

int shacira_pack_sum(int64_t num_samples, int64_t num_packs, int channels, const float *x, const int64_t *pack_start,
                     float *out, void *stream) {
    if (int rc = pack_args_ok(num_samples, num_packs, channels)) return rc;
    if (num_packs == 0) return 0;
    if (!pack_start || !out || (num_samples > 0 && !x)) return SHACIRA_EINVAL;
    return (int)pack_sum_launch(false, num_packs, channels, x, pack_start, out, (hipStream_t)stream);
}

int shacira_pack_broadcast(int64_t num_samples, int64_t num_packs, int channels, const float *per_pack,
                           const int64_t *pack_start, float *out, void *stream) {
    if (int rc = pack_args_ok(num_samples, num_packs, channels)) return rc;
    if (num_packs == 0 || num_samples == 0) return 0;
    if (!pack_start || !out || !per_pack) return SHACIRA_EINVAL;
    return (int)pack_sum_launch(true, num_packs, channels, per_pack, pack_start, out, (hipStream_t)stream);
}

static int march_args_ok(int64_t num_rays, const float *origins, const float *dirs, const uint8_t *occ, int level) {
    if (num_rays < 0 || level < 0 || level > 10) return SHACIRA_EINVAL;
    if (num_rays > 0 && (!origins || !dirs || !occ)) return SHACIRA_EINVAL;
    return 0;
}

int shacira_raymarch_ray_count(int64_t num_rays, int num_samples, const float *origins, const float *dirs,
                               float dist_min, float dist_max, const float *lin, const float *jitter,
                               const uint8_t *occupancy, int level, int32_t *counts, void *stream) {
    if (int rc = march_args_ok(num_rays, origins, dirs, occupancy, level)) return rc;
    if (num_samples < 1 || (num_rays > 0 && (!lin || !jitter || !counts))) return SHACIRA_EINVAL;
    return (int)raymarch_ray_launch(false, num_rays, num_samples, origins, dirs, dist_min, dist_max, lin, jitter,
                                    occupancy, level, counts, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    INT64_MAX, (hipStream_t)stream);
}

int shacira_raymarch_ray_emit(int64_t num_rays, int num_samples, const float *origins, const float *dirs,
                              float dist_min, float dist_max, const float *lin, const float *jitter,
                              const uint8_t *occupancy, int level, const int64_t *offsets, int64_t *ridx,
                              float *samples, float *depth, float *deltas, uint8_t *boundary, void *stream) {
    if (int rc = march_args_ok(num_rays, origins, dirs, occupancy, level)) return rc;
    if (num_samples < 1 || (num_rays > 0 && (!lin || !jitter || !offsets))) return SHACIRA_EINVAL;
    return (int)raymarch_ray_launch(true, num_rays, num_samples, origins, dirs, dist_min, dist_max, lin, jitter,
                                    occupancy, level, nullptr, offsets, ridx, samples, depth, deltas, boundary,
                                    INT64_MAX, (hipStream_t)stream);
}

int shacira_raymarch_ray_emit_capped(int64_t num_rays, int num_samples, const float *origins, const float *dirs,
                                     float dist_min, float dist_max, const float *lin, const float *jitter,
                                     const uint8_t *occupancy, int level, const int64_t *offsets, int64_t capacity,
                                     int64_t *ridx, float *samples, float *depth, float *deltas, uint8_t *boundary,
                                     void *stream) {
    if (int rc = march_args_ok(num_rays, origins, dirs, occupancy, level)) return rc;
    if (num_samples < 1 || capacity < 0 || (num_rays > 0 && (!lin || !jitter || !offsets))) return SHACIRA_EINVAL;
    return (int)raymarch_ray_launch(true, num_rays, num_samples, origins, dirs, dist_min, dist_max, lin, jitter,
                                    occupancy, level, nullptr, offsets, ridx, samples, depth, deltas, boundary,
                                    capacity, (hipStream_t)stream);
}

int shacira_raytrace_dense_count(int64_t num_rays, const float *origins, const float *dirs, const uint8_t *occupancy,
                                 int level, int32_t *counts, void *stream) {
    if (int rc = march_args_ok(num_rays, origins, dirs, occupancy, level)) return rc;
    if (num_rays > 0 && !counts) return SHACIRA_EINVAL;
    return (int)raytrace_dense_launch(false, num_rays, origins, dirs, occupancy, level, counts, nullptr, nullptr,
                                      nullptr, nullptr, (hipStream_t)stream);
}

int shacira_raytrace_dense_emit(int64_t num_rays, const float *origins, const float *dirs, const uint8_t *occupancy,
                                int level, const int64_t *offsets, int32_t *ridx, int32_t *pidx, float *depth,
                                void *stream) {
    if (int rc = march_args_ok(num_rays, origins, dirs, occupancy, level)) return rc;
    if (num_rays > 0 && !offsets) return SHACIRA_EINVAL;
    return (int)raytrace_dense_launch(true, num_rays, origins, dirs, occupancy, level, nullptr, offsets, ridx, pidx,
                                      depth, (hipStream_t)stream);
}

// rows of `capacity` belong to ceil(capacity / num_samples) nuggets of (ray uint32, entry fp32, exit fp32)
static bool voxel_sizes_ok(int64_t capacity, int num_samples) {
    return num_samples >= 1 && num_samples <= (1 << 24) && capacity >= 0 && capacity <= (int64_t)1 << 38;
}

size_t shacira_raymarch_voxel_workspace_bytes(int64_t capacity, int num_samples) {
    if (!voxel_sizes_ok(capacity, num_samples)) return 0;
    return (size_t)((capacity + num_samples - 1) / num_samples) * 12;
}

int shacira_raymarch_voxel_emit(int64_t num_rays, int num_samples, const float *origins, const float *dirs,
                                const uint8_t *occupancy, int level, const int64_t *offsets, uint64_t seed, int64_t step,
                                const int64_t *step_dev, int64_t capacity, void *workspace, size_t workspace_bytes,
                                int64_t *ridx, float *samples, float *depth, float *deltas, uint8_t *boundary,
                                void *stream) {
    if (int rc = march_args_ok(num_rays, origins, dirs, occupancy, level)) return rc;
    if (num_rays >= (int64_t)1 << 32 || !voxel_sizes_ok(capacity, num_samples)) return SHACIRA_EINVAL;
    if (num_rays == 0 || capacity == 0) return 0;
    if (!offsets || !ridx || !samples || !depth || !deltas || !boundary) return SHACIRA_EINVAL;
    if (!workspace || workspace_bytes < shacira_raymarch_voxel_workspace_bytes(capacity, num_samples))
        return SHACIRA_EWORKSPACE;
    return (int)raymarch_voxel_launch(num_rays, num_samples, origins, dirs, occupancy, level, offsets, seed, step, step_dev,
                                      capacity, workspace, ridx, samples, depth, deltas, boundary, (hipStream_t)stream);
}

size_t shacira_entropy_bits_workspace_bytes(int64_t, int) { return latent_workspace_bytes(); }

int shacira_entropy_bits_forward(int64_t num_rows, int latent_dim, int num_layers, const float *latent,
                                 const float *noise, const float *params, float *total_bits, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    if (num_rows < 0 || latent_dim < 1 || num_layers < 1 || num_layers > 4) return SHACIRA_EINVAL;
    if (!entropy_supported(latent_dim)) return SHACIRA_EDTYPE;
    if (!workspace || workspace_bytes < latent_workspace_bytes()) return SHACIRA_EWORKSPACE;
    if (!params || !total_bits || (num_rows > 0 && !latent)) return SHACIRA_EINVAL;
    EntropyArgs a{};
    a.latent = latent; a.noise = noise; a.params = params; a.num_layers = num_layers; a.total_bits = total_bits;
    a.partials = static_cast<double *>(workspace); a.rows = num_rows;
    return (int)entropy_dispatch(false, latent_dim, a, (hipStream_t)stream);
}

int shacira_entropy_bits_backward(int64_t num_rows, int latent_dim, int num_layers, const float *latent,
                                  const float *noise, const float *params, const float *grad_total_bits,
                                  float *grad_latent, float *grad_params, void *workspace, size_t workspace_bytes,
                                  void *stream) {
    if (num_rows < 0 || latent_dim < 1 || num_layers < 1 || num_layers > 4) return SHACIRA_EINVAL;
    if (!entropy_supported(latent_dim)) return SHACIRA_EDTYPE;
    if (!workspace || workspace_bytes < latent_workspace_bytes()) return SHACIRA_EWORKSPACE;
    if (!params || !grad_total_bits || (num_rows > 0 && !latent)) return SHACIRA_EINVAL;
    EntropyArgs a{};
    a.latent = latent; a.noise = noise; a.params = params; a.num_layers = num_layers; a.grad_total = grad_total_bits;
    a.grad_latent = grad_latent; a.grad_params = grad_params;
    a.partials = static_cast<double *>(workspace); a.rows = num_rows;
    return (int)entropy_dispatch(true, latent_dim, a, (hipStream_t)stream);
}

int shacira_adam_step(int64_t numel, float *param, float *grad, float *exp_avg, float *exp_avg_sq, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int step, int zero_grad, void *stream) {
    if (numel < 0 || step < 1) return SHACIRA_EINVAL;
    if (numel > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)) return SHACIRA_EINVAL;
    if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f)) return SHACIRA_EINVAL;
    return (int)adam_step_launch(param, grad, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay, step,
                                 nullptr, zero_grad, (hipStream_t)stream);
}

int shacira_adam_step_capturable(int64_t numel, float *param, float *grad, float *exp_avg, float *exp_avg_sq, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, const int32_t *step_dev,
                                 int zero_grad, void *stream) {
    if (numel < 0 || !step_dev) return SHACIRA_EINVAL;
    if (numel > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)) return SHACIRA_EINVAL;
    if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f)) return SHACIRA_EINVAL;
    return (int)adam_step_launch(param, grad, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay, 1,
                                 step_dev, zero_grad, (hipStream_t)stream);
}

int shacira_adam_step_multi_scaled(int num_tensors, const int64_t *numel_host, float *const *param, float *const *grad,
                                   float *const *exp_avg, float *const *exp_avg_sq, const float *lr_host,
                                   const float *weight_decay_host, float beta1, float beta2, float eps, int step,
                                   const int32_t *step_dev, int zero_grad, const float *grad_scale_dev,
                                   const float *found_inf_dev, void *stream) {
    if (num_tensors < 0 || num_tensors > 32) return SHACIRA_EINVAL;
    if (num_tensors == 0) return 0;
    if (!numel_host || !param || !grad || !exp_avg || !exp_avg_sq || !lr_host || !weight_decay_host)
        return SHACIRA_EINVAL;
    if (!step_dev && step < 1) return SHACIRA_EINVAL;
    if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f)) return SHACIRA_EINVAL;
    for (int t = 0; t < num_tensors; ++t)
        if (numel_host[t] < 0 || (numel_host[t] > 0 && (!param[t] || !grad[t] || !exp_avg[t] || !exp_avg_sq[t])))
            return SHACIRA_EINVAL;
    return (int)adam_multi_launch(num_tensors, param, grad, exp_avg, exp_avg_sq, numel_host, lr_host,
                                  weight_decay_host, beta1, beta2, eps, step, step_dev, grad_scale_dev, found_inf_dev,
                                  zero_grad, (hipStream_t)stream);
}

int shacira_adam_step_multi(int num_tensors, const int64_t *numel_host, float *const *param, float *const *grad,
                            float *const *exp_avg, float *const *exp_avg_sq, const float *lr_host,
                            const float *weight_decay_host, float beta1, float beta2, float eps, int step,
                            const int32_t *step_dev, int zero_grad, void *stream) {
    return shacira_adam_step_multi_scaled(num_tensors, numel_host, param, grad, exp_avg, exp_avg_sq, lr_host,
                                          weight_decay_host, beta1, beta2, eps, step, step_dev, zero_grad, nullptr,
                                          nullptr, stream);
}

int shacira_rmsprop_step_multi(int num_tensors, const int64_t *numel_host, float *const *param, float *const *grad,
                               float *const *square_avg, float *const *momentum_buf, const float *lr_host,
                               const float *weight_decay_host, float alpha, float eps, float momentum,
                               const float *grad_scale_dev, const float *found_inf_dev, int zero_grad, void *stream) {
    if (num_tensors < 0 || num_tensors > 32) return SHACIRA_EINVAL;
    if (num_tensors == 0) return 0;
    if (!numel_host || !param || !grad || !square_avg || !lr_host || !weight_decay_host) return SHACIRA_EINVAL;
    if (!(alpha >= 0.0f) || !(eps >= 0.0f) || !(momentum >= 0.0f)) return SHACIRA_EINVAL;
    if (momentum != 0.0f && !momentum_buf) return SHACIRA_EINVAL;
    for (int t = 0; t < num_tensors; ++t)
        if (numel_host[t] < 0 || (numel_host[t] > 0 && (!param[t] || !grad[t] || !square_avg[t] ||
                                                        (momentum != 0.0f && !momentum_buf[t]))))
            return SHACIRA_EINVAL;
    return (int)rmsprop_multi_launch(num_tensors, param, grad, square_avg, momentum_buf, numel_host, lr_host,
                                     weight_decay_host, alpha, eps, momentum, grad_scale_dev, found_inf_dev, zero_grad,
                                     (hipStream_t)stream);
}

int shacira_stream_probe(int kind, const void *src, void *dst, size_t bytes, void *stream) {
    if (kind < 0 || kind > 2 || (bytes & 15u)) return SHACIRA_EINVAL;
    if (bytes == 0) return 0;
    if ((kind != 1 && !src) || (kind != 0 && !dst)) return SHACIRA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) return SHACIRA_EINVAL;
    return (int)stream_probe_launch(kind, src, dst, bytes, kind == 0 ? static_cast<uint32_t *>(dst) : nullptr,
                                    (hipStream_t)stream);
}

int shacira_mlp_supported(int in_dim, int hidden_dim, int num_hidden, int out_dim) {
    options_snapshot();
    return mlp_supported(in_dim, hidden_dim, num_hidden, out_dim) ? 1 : 0;
}

size_t shacira_mlp_backward_workspace_bytes(int in_dim, int hidden_dim, int num_hidden, int out_dim) {
    options_snapshot();
    return mlp_supported(in_dim, hidden_dim, num_hidden, out_dim)
               ? mlp_workspace_bytes(in_dim, hidden_dim, num_hidden, out_dim) : 0;
}

// rows of 4n floats are read and written as float4 (mlp.hip load_row_in, mlp_mfma.hip load_input / store_rows)
static bool mlp_row_pointer_ok(const void *p, int row_floats) {
    return row_floats % 4 != 0 || (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

int shacira_mlp_forward(int64_t num_rows, int in_dim, int hidden_dim, int num_hidden, int out_dim, const float *x,
                        const float *params, float *y, void *stream) {
    options_snapshot();
    if (num_rows < 0) return SHACIRA_EINVAL;
    if (!mlp_supported(in_dim, hidden_dim, num_hidden, out_dim)) return SHACIRA_EDTYPE;
    if (num_rows == 0) return 0;
    if (!x || !params || !y) return SHACIRA_EINVAL;
    if (!mlp_row_pointer_ok(x, in_dim) || !mlp_row_pointer_ok(y, out_dim)) return SHACIRA_EINVAL;
    return (int)mlp_dispatch(false, in_dim, hidden_dim, num_hidden, out_dim, num_rows, x, params, y, nullptr, nullptr,
                             nullptr, nullptr, (hipStream_t)stream);
}

int shacira_mlp_backward(int64_t num_rows, int in_dim, int hidden_dim, int num_hidden, int out_dim, const float *x,
                         const float *params, const float *grad_y, float *grad_x, float *grad_params, void *workspace,
                         size_t workspace_bytes, void *stream) {
    options_snapshot();
    if (num_rows < 0) return SHACIRA_EINVAL;
    if (!mlp_supported(in_dim, hidden_dim, num_hidden, out_dim)) return SHACIRA_EDTYPE;
    if (!workspace || workspace_bytes < mlp_workspace_bytes(in_dim, hidden_dim, num_hidden, out_dim))
        return SHACIRA_EWORKSPACE;
    if (!params || !grad_params || (num_rows > 0 && (!x || !grad_y))) return SHACIRA_EINVAL;
    if (num_rows > 0 && (!mlp_row_pointer_ok(x, in_dim) || !mlp_row_pointer_ok(grad_x, in_dim))) return SHACIRA_EINVAL;
    return (int)mlp_dispatch(true, in_dim, hidden_dim, num_hidden, out_dim, num_rows, x, params, nullptr, grad_y,
                             grad_x, grad_params, static_cast<double *>(workspace), (hipStream_t)stream);
}

}  // extern "C"
