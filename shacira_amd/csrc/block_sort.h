// block_sort.h -- the counting sort of a batch's samples by spatial block, shared by the sorted backward passes of
// triplane.hip and octree.hip. The caller zeroes the block histogram (its own zero kernel, next to its
// gradients); block_sort_launch then issues, on the caller's stream and without host sync or allocation,
//
//   bin<RANK = false>   histogram of the samples by block
//   scan                one workgroup: start[b], ustart[b], and the histogram rewritten as the ranking cursor
//   bin<RANK = true>    every sample's slot in the sorted order
//
// and the caller's accumulation kernel, one workgroup per unit, finds its samples with block_sort_unit. A unit is up to
// CHUNK sorted samples of one block. What a block is (and the digit order of its id) belongs to the operator: a BlockOf
// functor, trivially copyable and passed by value, with
//   __device__ uint32_t operator()(const float *coords, int64_t i) const    // < nbins
#pragma once
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace shacira {

constexpr int kBlockSortLdsBins = 4096;        // histogram / ranking in LDS up to this many blocks, global atomics above
constexpr int kBlockSortMaxBlocksAxis = 64;    // cap of the sort's blocks per axis (262 144 blocks)

// RANK = false: block histogram; RANK = true: each sample's slot in the sorted order (per-workgroup counts in LDS, one global
// reservation per (workgroup, block)). Order inside a block is not fixed: the float sums that follow are not either.
template <int CHUNK, bool RANK, class BlockOf>
__global__ __launch_bounds__(256) void block_sort_bin_kernel(BlockOf block_of, int nbins, const float *__restrict__ coords,
                                                             uint32_t *__restrict__ counter, uint32_t *__restrict__ sorted,
                                                             int64_t N) {
    __shared__ uint32_t lcount[kBlockSortLdsBins];
    __shared__ uint32_t lbase[kBlockSortLdsBins];
    const bool lds = nbins <= kBlockSortLdsBins;
    const int64_t s0 = (int64_t)blockIdx.x * CHUNK;
    const int64_t s1 = s0 + CHUNK < N ? s0 + CHUNK : N;
    if (lds) {
        for (int b = threadIdx.x; b < nbins; b += blockDim.x) lcount[b] = 0u;
        __syncthreads();
    }
    constexpr int kPer = CHUNK / 256;
    uint32_t bin[kPer], rank[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int64_t i = s0 + (int64_t)k * 256 + threadIdx.x;
        bin[k] = 0u;
        rank[k] = 0u;
        if (i >= s1) continue;
        bin[k] = block_of(coords, i);
        if (lds) rank[k] = atomicAdd(&lcount[bin[k]], 1u);
        else rank[k] = atomicAdd(&counter[bin[k]], 1u);
    }
    if (!lds) {
        if constexpr (RANK) {
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const int64_t i = s0 + (int64_t)k * 256 + threadIdx.x;
                if (i < s1) sorted[rank[k]] = (uint32_t)i;
            }
        }
        return;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) {
        const uint32_t n = lcount[b];
        if (n) lbase[b] = atomicAdd(&counter[b], n);
    }
    if constexpr (RANK) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int64_t i = s0 + (int64_t)k * 256 + threadIdx.x;
            if (i < s1) sorted[lbase[bin[k]] + rank[k]] = (uint32_t)i;
        }
    }
}

// one workgroup: exclusive scan of the histogram -> start[b] (and the ranking cursor, the same values), units of CHUNK
// samples per block -> ustart[b]; start[nbins] = number of samples, ustart[nbins] = number of units
template <int CHUNK>
__global__ __launch_bounds__(1024) void block_sort_scan_kernel(int nbins, uint32_t *__restrict__ hist,
                                                               uint32_t *__restrict__ start,
                                                               uint32_t *__restrict__ ustart) {
    __shared__ uint32_t ws[2][1024];
    const int T = 1024;
    const int per = (nbins + T - 1) / T;
    const int b0 = std::min((int)threadIdx.x * per, nbins);
    const int b1 = b0 + per < nbins ? b0 + per : nbins;
    uint32_t s = 0, u = 0;
    for (int b = b0; b < b1; ++b) {
        s += hist[b];
        u += (hist[b] + CHUNK - 1) / CHUNK;
    }
    ws[0][threadIdx.x] = s;
    ws[1][threadIdx.x] = u;
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {   // Hillis-Steele inclusive scan
        uint32_t vs = 0, vu = 0;
        if ((int)threadIdx.x >= off) {
            vs = ws[0][threadIdx.x - off];
            vu = ws[1][threadIdx.x - off];
        }
        __syncthreads();
        ws[0][threadIdx.x] += vs;
        ws[1][threadIdx.x] += vu;
        __syncthreads();
    }
    s = ws[0][threadIdx.x] - s;
    u = ws[1][threadIdx.x] - u;
    for (int b = b0; b < b1; ++b) {
        const uint32_t n = hist[b];
        start[b] = s;
        ustart[b] = u;
        hist[b] = s;   // the ranking pass's cursor
        s += n;
        u += (n + CHUNK - 1) / CHUNK;
    }
    if (threadIdx.x == T - 1) {
        start[nbins] = ws[0][T - 1];
        ustart[nbins] = ws[1][T - 1];
    }
}

// the block b and the sorted range [s0, s1) of accumulation unit `unit`; false: no such unit (the grid is an upper bound)
template <int CHUNK>
__device__ __forceinline__ bool block_sort_unit(uint32_t unit, int nbins, const uint32_t *__restrict__ start,
                                                const uint32_t *__restrict__ ustart, int &b, uint32_t &s0, uint32_t &s1) {
    if (unit >= ustart[nbins]) return false;
    int lo = 0, hi = nbins - 1;   // the block whose unit range holds `unit`: last b with ustart[b] <= unit
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ustart[mid] <= unit) lo = mid;
        else hi = mid - 1;
    }
    b = lo;
    s0 = start[b] + (unit - ustart[b]) * (uint32_t)CHUNK;
    s1 = s0 + CHUNK < start[b + 1] ? s0 + CHUNK : start[b + 1];
    return true;
}

// ------------------------------------------------------------------------------------------------------- host side
// workspace: hist, start, ustart ([nbins + 1] each) and sorted ([n]), each 256-byte aligned
inline size_t block_sort_align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline size_t block_sort_workspace_bytes(int nbins, int64_t n) {
    return 3 * block_sort_align256(((size_t)nbins + 1) * sizeof(uint32_t)) +
           block_sort_align256((size_t)n * sizeof(uint32_t));
}

struct BlockSortBuffers {
    uint32_t *hist, *start, *ustart, *sorted;
};

inline BlockSortBuffers block_sort_carve(void *workspace, int nbins) {
    char *w = static_cast<char *>(workspace);
    const size_t binb = block_sort_align256(((size_t)nbins + 1) * sizeof(uint32_t));
    return {reinterpret_cast<uint32_t *>(w), reinterpret_cast<uint32_t *>(w + binb),
            reinterpret_cast<uint32_t *>(w + 2 * binb), reinterpret_cast<uint32_t *>(w + 3 * binb)};
}

// sorts n > 0 samples (buf.hist zeroed earlier on the stream); returns the grid of the accumulation kernel: an upper bound
// of the number of units (each block rounds up once)
template <int CHUNK, class BlockOf>
inline uint32_t block_sort_launch(BlockOf block_of, const float *coords, int64_t n, int nbins, const BlockSortBuffers &buf,
                                  hipStream_t s) {
    const uint32_t chunks = (uint32_t)((n + CHUNK - 1) / CHUNK);
    hipLaunchKernelGGL((block_sort_bin_kernel<CHUNK, false, BlockOf>), dim3(chunks), dim3(256), 0, s, block_of, nbins,
                       coords, buf.hist, nullptr, n);
    hipLaunchKernelGGL((block_sort_scan_kernel<CHUNK>), dim3(1), dim3(1024), 0, s, nbins, buf.hist, buf.start, buf.ustart);
    hipLaunchKernelGGL((block_sort_bin_kernel<CHUNK, true, BlockOf>), dim3(chunks), dim3(256), 0, s, block_of, nbins,
                       coords, buf.hist, buf.sorted, n);
    return chunks + (uint32_t)nbins;
}

}  // namespace shacira
