// bwd_bin_call.h -- the binned hash-grid backward (hashgrid_bwd_bin.hip) as its dispatcher (hashgrid_bwd.hip) sees it.
//
// Everything the binned backward decides per call is decided once, by bin_resolve(), and travels in one host-only value, the
// BinCall: the workspace size, the carving, the plans and the launch sequence all read it and derive nothing again. A C-ABI
// call resolves once and uses the same value for its size check and for the launch. The struct is defined beside the plans it
// holds (hashgrid_bwd_bin.hip); the dispatcher keeps it in its own frame as raw storage (no allocation, no hidden state).
#pragma once

#include "internal.h"

namespace shacira {

struct BinCall;
struct BinCallBox {
    alignas(16) unsigned char raw[512];
};

bool bin_supported(int dim, const LevelTable &lt);
bool bin_all_direct(int dim, const LevelTable &lt);
// `sb`: the batch's plan (only its block grid is read) or NULL; `zero_table`: the call covers all levels and zeroes the table;
// `grad_aligned`: 16-byte aligned grad_output. Without a plan the last two do not matter.
const BinCall &bin_resolve(BinCallBox &box, int dim, int dtype, const LevelTable &lt, int64_t n, const SortedBatch *sb,
                           bool zero_table, bool grad_aligned);
size_t bin_workspace_bytes(const BinCall &call, const LevelTable &lt);
float *bin_acc32(const BinCall &call, const LevelTable &lt, void *workspace);   // fp16 tables: the fp32 accumulation image
hipError_t bin_backward(const BinCall &call, const LevelTable &lt, const int32_t *first_idx, const float *coords,
                        const void *grad_out, float *acc, void *workspace, hipStream_t s, bool zero_table, void *half_table,
                        bool *converted, const SortedBatch *sb);

}  // namespace shacira
