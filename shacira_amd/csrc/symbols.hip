// symbols.hip -- integer symbol statistics of the rounded latents (gfx950) + the host-side range coder.
//
// Reference: LatentGrid.size (wisp/models/grids/latent_grid.py:138-174) rounds every latent channel, runs
// torch.unique(return_counts=True) (a device-wide sort, once per epoch and per channel) and turns the counts into an
// entropy estimate or, with torchac, into an arithmetic-coded byte stream. Here:
//   symbol_range      per channel min / max of (int)rint(latent)            one streaming pass, int32 atomics
//   symbol_histogram  per channel counts over [lo, lo + nbins)              one streaming pass, LDS-private bins
//   range coder       static-model byte-wise range coder on the HOST (the reference also codes on the CPU:
//                     `cdf.detach().cpu()`); carry-propagating 40-bit range / 16-bit frequency scale.
//   rans64            64-lane interleaved rANS over the same model (format: include/shacira_hip.h): a host coder and
//                     device kernels, one wavefront per (block, channel), that write the same bytes. The encoder reads
//                     the fp32 latents, the decoder writes them; the table never leaves the GPU, only the bytes do.
// Integer work: results must be exact.
#include <vector>

#include "internal.h"

namespace shacira {

constexpr int kSymMaxLD = 16;
constexpr int kSymThreads = 256;
constexpr int kSymLdsBins = 12288;   // 48 KiB of private uint32 bins per workgroup

__device__ __forceinline__ int32_t to_symbol(float v) {
    // torch.round (half to even) then .long(); clamped so that lo/hi arithmetic cannot overflow. NaN -> 0.
    const float r = rintf(v);
    const float c = fminf(fmaxf(r, -1073741824.0f), 1073741824.0f);   // fmaxf / fminf drop a NaN operand: test r, not c
    return (r == r) ? (int32_t)c : 0;
}

__global__ void symbol_range_init_kernel(int32_t *__restrict__ minmax, int ld) {
    const int c = threadIdx.x;
    if (c < ld) {
        minmax[2 * c] = INT32_MAX;
        minmax[2 * c + 1] = INT32_MIN;
    }
}

__global__ __launch_bounds__(kSymThreads) void symbol_range_kernel(const float *__restrict__ latent, int64_t rows,
                                                                   int ld, int32_t *__restrict__ minmax) {
    __shared__ int32_t s_mm[2 * kSymMaxLD];
    if (threadIdx.x < 2 * kSymMaxLD) s_mm[threadIdx.x] = (threadIdx.x & 1) ? INT32_MIN : INT32_MAX;
    __syncthreads();
    // flat walk: consecutive threads read consecutive floats; a thread's channel changes by (stride % ld) per step
    const int64_t total = rows * ld;
    const int64_t stride = (int64_t)gridDim.x * kSymThreads;
    int32_t mn[kSymMaxLD], mx[kSymMaxLD];
#pragma unroll
    for (int c = 0; c < kSymMaxLD; ++c) {
        mn[c] = INT32_MAX;
        mx[c] = INT32_MIN;
    }
    for (int64_t e = (int64_t)blockIdx.x * kSymThreads + threadIdx.x; e < total; e += stride) {
        const int c = (int)(e % ld);
        const int32_t s = to_symbol(latent[e]);
#pragma unroll
        for (int k = 0; k < kSymMaxLD; ++k)   // register-resident select instead of a dynamically indexed array
            if (k == c) {
                mn[k] = s < mn[k] ? s : mn[k];
                mx[k] = s > mx[k] ? s : mx[k];
            }
    }
#pragma unroll
    for (int c = 0; c < kSymMaxLD; ++c) {
        if (c < ld && mn[c] <= mx[c]) {
            atomicMin(&s_mm[2 * c], mn[c]);
            atomicMax(&s_mm[2 * c + 1], mx[c]);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * ld) {
        const int32_t v = s_mm[threadIdx.x];
        if (threadIdx.x & 1) { if (v != INT32_MIN) atomicMax(&minmax[threadIdx.x], v); }
        else                 { if (v != INT32_MAX) atomicMin(&minmax[threadIdx.x], v); }
    }
}

// counts[c][s - lo[c]] += 1 ; symbols outside [lo, lo + nbins) are ignored (cannot happen with lo/nbins from
// symbol_range). LDS-private bins when ld * nbins fits, flushed with one global atomic per non-empty bin.
template <bool LDS>
__global__ __launch_bounds__(kSymThreads) void symbol_histogram_kernel(const float *__restrict__ latent, int64_t rows,
                                                                       int ld, const int32_t *__restrict__ minmax,
                                                                       int nbins,
                                                                       unsigned long long *__restrict__ counts) {
    extern __shared__ uint32_t s_bins[];
    __shared__ int32_t s_lo[kSymMaxLD];
    if ((int)threadIdx.x < ld) s_lo[threadIdx.x] = minmax[2 * threadIdx.x];
    const int nb_all = ld * nbins;
    if constexpr (LDS)
        for (int k = threadIdx.x; k < nb_all; k += kSymThreads) s_bins[k] = 0;
    __syncthreads();
    const int64_t total = rows * ld;
    const int64_t stride = (int64_t)gridDim.x * kSymThreads;
    for (int64_t e = (int64_t)blockIdx.x * kSymThreads + threadIdx.x; e < total; e += stride) {
        const int c = (int)(e % ld);
        const int64_t b = (int64_t)to_symbol(latent[e]) - (int64_t)s_lo[c];
        if (b < 0 || b >= nbins) continue;
        if constexpr (LDS) atomicAdd(&s_bins[c * nbins + (int)b], 1u);
        else atomicAdd(&counts[(size_t)c * nbins + (size_t)b], 1ull);
    }
    if constexpr (LDS) {
        __syncthreads();
        for (int k = threadIdx.x; k < nb_all; k += kSymThreads) {
            const uint32_t v = s_bins[k];
            if (v) atomicAdd(&counts[k], (unsigned long long)v);
        }
    }
}

static uint32_t stream_blocks(int64_t total) {
    int64_t b = (total + kSymThreads * 8 - 1) / (kSymThreads * 8);
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (uint32_t)b;
}

bool symbols_supported(int ld) { return ld >= 1 && ld <= kSymMaxLD; }

hipError_t symbol_range_launch(const float *latent, int64_t rows, int ld, int32_t *minmax, hipStream_t s) {
    hipLaunchKernelGGL(symbol_range_init_kernel, dim3(1), dim3(64), 0, s, minmax, ld);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || rows == 0) return e;
    hipLaunchKernelGGL(symbol_range_kernel, dim3(stream_blocks(rows * ld)), dim3(kSymThreads), 0, s, latent, rows, ld,
                       minmax);
    return hipGetLastError();
}

hipError_t symbol_histogram_launch(const float *latent, int64_t rows, int ld, const int32_t *minmax, int nbins,
                                   uint64_t *counts, hipStream_t s) {
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)ld * nbins * sizeof(uint64_t), s);
    if (e != hipSuccess || rows == 0) return e;
    const uint32_t blocks = stream_blocks(rows * ld);
    auto *c = reinterpret_cast<unsigned long long *>(counts);
    if ((int64_t)ld * nbins <= kSymLdsBins)
        hipLaunchKernelGGL(symbol_histogram_kernel<true>, dim3(blocks), dim3(kSymThreads),
                           (size_t)ld * nbins * sizeof(uint32_t), s, latent, rows, ld, minmax, nbins, c);
    else
        hipLaunchKernelGGL(symbol_histogram_kernel<false>, dim3(blocks), dim3(kSymThreads), 0, s, latent, rows, ld,
                           minmax, nbins, c);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ range coder (host)
// Byte-wise range coder with carry propagation (the construction used by LZMA's rc, generalised from binary to
// multi-symbol models): 40-bit range (renormalised byte-wise above 2^32, so range / 2^16 keeps >= 16 significant bits
// and the truncation loss stays below 3e-5 bit per symbol -- it matters for near-deterministic channels), 41-bit low
// with carry, frequencies scaled to a total of 2^16 (every coded symbol has freq >= 1). Static model: the caller
// supplies the frequency table, which also goes into the container.
constexpr uint32_t kRcTotalBits = 16;
constexpr uint64_t kRcRangeInit = (1ull << 40) - 1;
constexpr uint64_t kRcTop = 1ull << 32;
constexpr uint64_t kRcMask40 = (1ull << 40) - 1;

int rc_check_model(const uint32_t *freq, int nsym) {
    if (!freq || nsym < 1 || nsym > (1 << kRcTotalBits)) return SHACIRA_EINVAL;
    uint64_t sum = 0;
    for (int k = 0; k < nsym; ++k) sum += freq[k];
    return sum == (1u << kRcTotalBits) ? 0 : SHACIRA_EINVAL;
}

size_t rc_encode_bound(int64_t n) { return (size_t)n * 2 + 16; }  // >= 16 bits per symbol is the worst case (freq 1)

int rc_encode(const int32_t *sym, int64_t n, const uint32_t *freq, int nsym, uint8_t *out, size_t cap, size_t *len) {
    int rc = rc_check_model(freq, nsym);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !sym) || !out || !len) return SHACIRA_EINVAL;
    std::vector<uint32_t> cum((size_t)nsym + 1, 0);
    for (int k = 0; k < nsym; ++k) cum[k + 1] = cum[k] + freq[k];
    uint64_t low = 0;
    uint64_t range = kRcRangeInit;
    uint8_t cache = 0;
    uint64_t cache_size = 1;
    size_t pos = 0;
    bool overflow = false;
    auto put = [&](uint8_t b) {
        if (pos < cap) out[pos] = b; else overflow = true;
        ++pos;
    };
    auto shift_low = [&]() {
        if ((low & kRcMask40) < (0xFFull << 32) || (low >> 40) != 0) {
            const uint8_t carry = (uint8_t)(low >> 40);
            uint8_t temp = cache;
            do {
                put((uint8_t)(temp + carry));
                temp = 0xFF;
            } while (--cache_size != 0);
            cache = (uint8_t)((low >> 32) & 0xFF);
        }
        ++cache_size;
        low = (low & 0xFFFFFFFFull) << 8;
    };
    for (int64_t i = 0; i < n; ++i) {
        const int32_t s = sym[i];
        if (s < 0 || s >= nsym || freq[s] == 0) return SHACIRA_EINVAL;   // symbol without code space
        const uint64_t r = range >> kRcTotalBits;
        low += r * cum[s];
        range = r * freq[s];
        while (range < kRcTop) {
            range <<= 8;
            shift_low();
        }
    }
    for (int k = 0; k < 6; ++k) shift_low();
    *len = pos;
    return overflow ? SHACIRA_EWORKSPACE : 0;
}

int rc_decode(const uint8_t *in, size_t len, const uint32_t *freq, int nsym, int64_t n, int32_t *sym) {
    int rc = rc_check_model(freq, nsym);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!sym || !in))) return SHACIRA_EINVAL;
    std::vector<uint32_t> cum((size_t)nsym + 1, 0);
    for (int k = 0; k < nsym; ++k) cum[k + 1] = cum[k] + freq[k];
    std::vector<uint16_t> lookup((size_t)1 << kRcTotalBits);
    if (nsym > 65536) return SHACIRA_EINVAL;
    for (int k = 0; k < nsym; ++k)
        for (uint32_t v = cum[k]; v < cum[k + 1]; ++v) lookup[v] = (uint16_t)k;
    size_t pos = 0;
    auto next = [&]() -> uint64_t { return pos < len ? in[pos++] : (pos++, 0u); };
    uint64_t code = 0, range = kRcRangeInit;
    (void)next();   // the encoder's first byte is its initial cache (always 0)
    for (int k = 0; k < 5; ++k) code = (code << 8) | next();
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t r = range >> kRcTotalBits;
        uint64_t v = code / r;
        if (v >= (1u << kRcTotalBits)) v = (1u << kRcTotalBits) - 1;
        const uint32_t s = lookup[v];
        code -= r * cum[s];
        range = r * freq[s];
        while (range < kRcTop) {
            code = (code << 8) | next();
            range <<= 8;
        }
        sym[i] = (int32_t)s;
    }
    return pos <= len + 5 ? 0 : SHACIRA_EINVAL;   // ran past the stream: truncated / wrong model
}

// ---------------------------------------------------------------------------------- interleaved rANS ("rans64")
// The format is stated in include/shacira_hip.h. 64 coder states per block advance in lockstep and share one stream of
// 16-bit words; a state x lives in [2^16, 2^32) and renormalises one word at a time. With the frequencies scaled to
// 2^16 (every coded f in [1, 65535]): the encoder emits at most ONE word per symbol (after the shift x < 2^16 <= f << 16),
// x / f >= 1 before the update (emitted: x >> 16 >= f; not emitted: x >= 2^16 > f) so the new state is >= 2^16, and
// x < f << 16 keeps it below 2^32. The decoder's update leaves x >= 1, so one word brings it back above 2^16.
// `x / f` and `x % f` are the language's unsigned 32-bit operators on both sides: exact by definition (the device
// compiler expands them into a reciprocal estimate with integer correction steps, not into a float quotient).
constexpr int kRansLanes = 64;
constexpr uint32_t kRansLow = 1u << 16;
constexpr int kRansMaxSteps = 1 << 16;
constexpr int kRansBlockHeader = 4 + 4 * kRansLanes;   // n_b + the final states: the flush, 260 bytes per block
constexpr int kRansLdsCdf = 4096;                      // cdf entries (nbins + 1) searched from LDS: 16 KiB per wave

bool rans_steps_ok(int steps) { return steps >= 1 && steps <= kRansMaxSteps; }

int64_t rans_num_blocks(int64_t n, int steps) {
    const int64_t per = (int64_t)kRansLanes * steps;
    return (n + per - 1) / per;
}

// steps of block b that own at least one symbol (the others have no active lane and do nothing)
__host__ __device__ static inline int rans_live_steps(int64_t n, int64_t base, int steps) {
    const int64_t need = (n - base + kRansLanes - 1) / kRansLanes;
    return need < steps ? (int)need : steps;
}

static int rans_check_model(const uint32_t *freq, int nsym) {
    int rc = rc_check_model(freq, nsym);
    if (rc) return rc;
    for (int k = 0; k < nsym; ++k)
        if (freq[k] >= (1u << kRcTotalBits)) return SHACIRA_EINVAL;   // a single-symbol channel carries no payload
    return 0;
}

size_t rans_encode_bound(int64_t n, int steps) {
    return (size_t)rans_num_blocks(n, steps) * kRansBlockHeader + (size_t)n * 2;
}

static inline void put_le32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}
static inline uint32_t get_le32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

int rans_encode(const int32_t *sym, int64_t n, const uint32_t *freq, int nsym, int steps, uint8_t *out, size_t cap,
                size_t *len) {
    int rc = rans_check_model(freq, nsym);
    if (rc) return rc;
    if (!rans_steps_ok(steps) || n < 0 || (n > 0 && !sym) || !out || !len) return SHACIRA_EINVAL;
    for (int64_t i = 0; i < n; ++i)
        if (sym[i] < 0 || sym[i] >= nsym || freq[sym[i]] == 0) return SHACIRA_EINVAL;   // symbol without code space
    std::vector<uint32_t> cum((size_t)nsym + 1, 0);
    for (int k = 0; k < nsym; ++k) cum[k + 1] = cum[k] + freq[k];
    const int64_t nblocks = rans_num_blocks(n, steps);
    const size_t head = (size_t)nblocks * kRansBlockHeader;
    const bool head_fits = head <= cap;
    size_t pos = head;
    bool overflow = !head_fits;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int64_t base = b * kRansLanes * steps;
        uint32_t x[kRansLanes];
        for (int l = 0; l < kRansLanes; ++l) x[l] = kRansLow;
        uint32_t nb = 0;
        for (int k = rans_live_steps(n, base, steps) - 1; k >= 0; --k) {
            for (int l = 0; l < kRansLanes; ++l) {   // lane order = word order; the lanes do not depend on each other
                const int64_t i = base + (int64_t)k * kRansLanes + l;
                if (i >= n) break;
                const uint32_t f = freq[sym[i]], c = cum[sym[i]];
                if (x[l] >= (f << 16)) {
                    if (pos + 2 <= cap) {
                        out[pos] = (uint8_t)x[l];
                        out[pos + 1] = (uint8_t)(x[l] >> 8);
                    } else {
                        overflow = true;
                    }
                    pos += 2;
                    ++nb;
                    x[l] >>= 16;
                }
                x[l] = ((x[l] / f) << 16) + (x[l] % f) + c;
            }
        }
        if (head_fits) {
            put_le32(out + 4 * b, nb);
            for (int l = 0; l < kRansLanes; ++l) put_le32(out + 4 * nblocks + 4 * (b * kRansLanes + l), x[l]);
        }
    }
    *len = pos;
    return overflow ? SHACIRA_EWORKSPACE : 0;
}

// Never indexes outside `in` / `sym`, whatever the bytes: the counts must add up to the words present, every state must be
// a legal one, and the read position may not pass the start of its block's words.
int rans_decode(const uint8_t *in, size_t len, const uint32_t *freq, int nsym, int64_t n, int steps, int32_t *sym) {
    int rc = rans_check_model(freq, nsym);
    if (rc) return rc;
    if (!rans_steps_ok(steps) || n < 0 || (n > 0 && (!sym || !in))) return SHACIRA_EINVAL;
    const int64_t nblocks = rans_num_blocks(n, steps);
    const size_t head = (size_t)nblocks * kRansBlockHeader;
    if (len < head || ((len - head) & 1)) return SHACIRA_EINVAL;
    const uint64_t nwords = (len - head) / 2;
    uint64_t sum = 0;
    for (int64_t b = 0; b < nblocks; ++b) sum += get_le32(in + 4 * b);
    if (sum != nwords) return SHACIRA_EINVAL;
    for (int64_t k = 0; k < nblocks * kRansLanes; ++k)
        if (get_le32(in + 4 * nblocks + 4 * k) < kRansLow) return SHACIRA_EINVAL;
    std::vector<uint32_t> cum((size_t)nsym + 1, 0);
    for (int k = 0; k < nsym; ++k) cum[k + 1] = cum[k] + freq[k];
    std::vector<uint16_t> lookup((size_t)1 << kRcTotalBits);
    for (int k = 0; k < nsym; ++k)
        for (uint32_t v = cum[k]; v < cum[k + 1]; ++v) lookup[v] = (uint16_t)k;
    const uint8_t *words = in + head;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int64_t base = b * kRansLanes * steps;
        uint32_t x[kRansLanes];
        for (int l = 0; l < kRansLanes; ++l) x[l] = get_le32(in + 4 * nblocks + 4 * (b * kRansLanes + l));
        const uint64_t nb = get_le32(in + 4 * b);
        uint64_t p = nb;
        const int live = rans_live_steps(n, base, steps);
        for (int k = 0; k < live; ++k) {
            uint64_t need = 0;
            for (int l = 0; l < kRansLanes; ++l) {
                const int64_t i = base + (int64_t)k * kRansLanes + l;
                if (i >= n) break;
                const uint32_t slot = x[l] & 0xFFFFu;
                const uint32_t s = lookup[slot];
                x[l] = freq[s] * (x[l] >> 16) + slot - cum[s];
                sym[i] = (int32_t)s;
                need += x[l] < kRansLow;
            }
            if (need > p) return SHACIRA_EINVAL;   // the block asks for more words than it holds
            p -= need;
            uint64_t r = p;
            for (int l = 0; l < kRansLanes; ++l) {
                if (base + (int64_t)k * kRansLanes + l >= n) break;
                if (x[l] < kRansLow) {
                    x[l] = (x[l] << 16) | words[2 * r] | ((uint32_t)words[2 * r + 1] << 8);
                    ++r;
                }
            }
        }
        if (p != 0) return SHACIRA_EINVAL;
        for (int l = 0; l < kRansLanes; ++l)
            if (x[l] != kRansLow) return SHACIRA_EINVAL;   // not the encoder's initial state: wrong bytes or model
        words += 2 * nb;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------- rans64 on the device
// One wavefront per (block, channel): the 64 lanes are the 64 coder states. The words a step emits / needs are placed
// with the 64-bit ballot of the lanes concerned: rank = mbcnt (set bits below the lane), count = popcount.
struct RansChannels {             // per channel, passed by value (validated on the host before the launch)
    int64_t payload[kSymMaxLD];   // byte offset of the channel payload in the packed buffer / container, multiple of 4
    int64_t words[kSymMaxLD];     // 16-bit words of the channel
    int32_t lo[kSymMaxLD];        // value of symbol 0
    int32_t nbins[kSymMaxLD];     // < 2: the channel carries no payload
};

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// encodes block blockIdx.x of channel blockIdx.y into its bound-sized slot (64 * steps words: one per symbol at most)
template <bool LDS>
__global__ __launch_bounds__(kRansLanes) void rans_encode_kernel(const float *__restrict__ latent, int64_t rows, int ld,
                                                                 RansChannels ch, const uint32_t *__restrict__ cdf,
                                                                 int cdf_stride, int steps, int64_t nblocks,
                                                                 uint32_t *__restrict__ counts,
                                                                 uint32_t *__restrict__ states,
                                                                 uint16_t *__restrict__ slots) {
    extern __shared__ uint32_t s_cdf[];
    const int c = blockIdx.y, lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int nbins = ch.nbins[c];
    const int64_t seg = (int64_t)c * nblocks + b;
    if (nbins < 2) {
        if (lane == 0) counts[seg] = 0;
        states[seg * kRansLanes + lane] = kRansLow;
        return;
    }
    const uint32_t *g_cdf = cdf + (size_t)c * cdf_stride;
    if constexpr (LDS) {
        for (int k = lane; k <= nbins; k += kRansLanes) s_cdf[k] = g_cdf[k];
        __syncthreads();
    }
    auto cdf_at = [&](int k) -> uint32_t {
        if constexpr (LDS) return s_cdf[k];
        else return g_cdf[k];
    };
    const int64_t lo = ch.lo[c];
    const int64_t base = b * kRansLanes * steps;
    uint16_t *slot = slots + (size_t)seg * kRansLanes * steps;
    auto value = [&](int k) -> float {   // 0 for an inactive lane: any symbol, it is not coded
        const int64_t i = base + (int64_t)k * kRansLanes + lane;
        return i < rows ? latent[i * ld + c] : 0.0f;
    };
    uint32_t x = kRansLow, n = 0;
    int k = rans_live_steps(rows, base, steps) - 1;
    float v = value(k);
    for (; k >= 0; --k) {
        const float v_next = k > 0 ? value(k - 1) : 0.0f;   // the load does not wait for the coder's dependent chain
        const bool active = base + (int64_t)k * kRansLanes + lane < rows;
        int64_t s = (int64_t)to_symbol(v) - lo;
        s = s < 0 ? 0 : (s > nbins - 1 ? nbins - 1 : s);     // inside the model whatever the table holds
        const uint32_t c0 = cdf_at((int)s);
        uint32_t f = cdf_at((int)s + 1) - c0;
        f = f == 0 ? 1u : f;                                 // a symbol the model lacks: wrong bytes, no fault
        const bool emit = active && (uint64_t)x >= ((uint64_t)f << 16);
        const unsigned long long mask = __ballot(emit);
        if (emit) {
            slot[n + lanes_below(mask)] = (uint16_t)x;       // adjacent lanes, adjacent words; n <= 64 * steps
            x >>= 16;
        }
        n += (uint32_t)__popcll(mask);
        if (active) x = ((x / f) << 16) + (x % f) + c0;
        v = v_next;
    }
    if (lane == 0) counts[seg] = n;
    states[seg * kRansLanes + lane] = x;
}

// moves a block's count, states and words to their place in the channel payload (block_start: exclusive prefix of counts)
__global__ __launch_bounds__(kSymThreads) void rans_pack_kernel(RansChannels ch, int steps, int64_t nblocks,
                                                                const uint32_t *__restrict__ counts,
                                                                const uint32_t *__restrict__ states,
                                                                const uint16_t *__restrict__ slots,
                                                                const int64_t *__restrict__ block_start,
                                                                uint8_t *__restrict__ out) {
    const int c = blockIdx.y;
    const int64_t b = blockIdx.x;
    if (ch.nbins[c] < 2) return;
    const int64_t seg = (int64_t)c * nblocks + b;
    uint8_t *pay = out + ch.payload[c];
    const int64_t total = ch.words[c];
    int64_t start = block_start[seg];
    start = start < 0 ? 0 : (start > total ? total : start);
    int64_t n = counts[seg];
    n = n > (int64_t)kRansLanes * steps ? (int64_t)kRansLanes * steps : n;
    n = n > total - start ? total - start : n;
    if (threadIdx.x == 0) reinterpret_cast<uint32_t *>(pay)[b] = counts[seg];
    if (threadIdx.x < kRansLanes)
        reinterpret_cast<uint32_t *>(pay + 4 * nblocks)[b * kRansLanes + threadIdx.x] =
            states[seg * kRansLanes + threadIdx.x];
    uint16_t *dst = reinterpret_cast<uint16_t *>(pay + (int64_t)kRansBlockHeader * nblocks) + start;
    const uint16_t *src = slots + (size_t)seg * kRansLanes * steps;
    for (int64_t i = threadIdx.x; i < n; i += kSymThreads) dst[i] = src[i];
}

// decodes block blockIdx.x of channel blockIdx.y straight into the fp32 [rows, ld] table. Word indices are clamped into
// the block's [0, n_b), the block's words into the channel's, the symbol into [0, nbins): corrupt bytes give wrong values
// and raise *error, never an access outside the container.
template <bool LDS>
__global__ __launch_bounds__(kRansLanes) void rans_decode_kernel(const uint8_t *__restrict__ data, RansChannels ch,
                                                                 const uint32_t *__restrict__ cdf, int cdf_stride,
                                                                 const int64_t *__restrict__ block_start, int steps,
                                                                 int64_t nblocks, int64_t rows, int ld,
                                                                 float *__restrict__ out, int32_t *__restrict__ error) {
    extern __shared__ uint32_t s_cdf[];
    const int c = blockIdx.y, lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int nbins = ch.nbins[c];
    const int32_t lo = ch.lo[c];
    const int64_t base = b * kRansLanes * steps;
    const int live = rans_live_steps(rows, base, steps);
    if (nbins < 2) {                                          // one symbol only: no payload, every row holds lo
        for (int k = 0; k < live; ++k) {
            const int64_t i = base + (int64_t)k * kRansLanes + lane;
            if (i < rows) out[i * ld + c] = (float)lo;
        }
        return;
    }
    const uint32_t *g_cdf = cdf + (size_t)c * cdf_stride;
    if constexpr (LDS) {
        for (int k = lane; k <= nbins; k += kRansLanes) s_cdf[k] = g_cdf[k];
        __syncthreads();
    }
    auto cdf_at = [&](int k) -> uint32_t {
        if constexpr (LDS) return s_cdf[k];
        else return g_cdf[k];
    };
    const uint8_t *pay = data + ch.payload[c];
    const int64_t total = ch.words[c];
    int64_t start = block_start[(int64_t)c * nblocks + b];
    start = start < 0 ? 0 : (start > total ? total : start);
    int64_t nb = reinterpret_cast<const uint32_t *>(pay)[b];
    nb = nb > total - start ? total - start : nb;
    const uint16_t *words = reinterpret_cast<const uint16_t *>(pay + (int64_t)kRansBlockHeader * nblocks) + start;
    uint32_t x = reinterpret_cast<const uint32_t *>(pay + 4 * nblocks)[b * kRansLanes + lane];
    bool bad = x < kRansLow;
    int64_t p = nb;
    for (int k = 0; k < live; ++k) {
        const int64_t i = base + (int64_t)k * kRansLanes + lane;
        const bool active = i < rows;
        if (active) {
            const uint32_t slot = x & 0xFFFFu;
            int a = 0, z = nbins - 1;                         // largest s in [0, nbins) with cdf[s] <= slot (cdf[0] = 0)
            while (a < z) {
                const int mid = (a + z + 1) >> 1;
                if (cdf_at(mid) <= slot) a = mid;
                else z = mid - 1;
            }
            const uint32_t c0 = cdf_at(a);
            x = (cdf_at(a + 1) - c0) * (x >> 16) + slot - c0;
            out[i * ld + c] = (float)(a + lo);
        }
        const bool need = active && x < kRansLow;
        const unsigned long long mask = __ballot(need);
        const int64_t n = __popcll(mask);
        bad = bad || n > p;
        if (need) {
            int64_t w = p - n + lanes_below(mask);
            w = w > nb - 1 ? nb - 1 : w;
            w = w < 0 ? 0 : w;
            x = (x << 16) | (nb > 0 ? (uint32_t)words[w] : 0u);
        }
        p -= n;
    }
    if (bad || p != 0 || x != kRansLow) atomicOr(error, 1);
}

static size_t rans_cdf_lds(const int32_t *nbins, int ld) {   // 0: some channel's cdf is too long, search global memory
    int most = 0;
    for (int c = 0; c < ld; ++c) most = nbins[c] > most ? nbins[c] : most;
    return most + 1 <= kRansLdsCdf ? (size_t)(most + 1) * sizeof(uint32_t) : 0;
}

static RansChannels rans_channels(int ld, const int32_t *lo, const int32_t *nbins, const int64_t *payload,
                                  const int64_t *words) {
    RansChannels ch = {};
    for (int c = 0; c < ld; ++c) {
        ch.lo[c] = lo ? lo[c] : 0;
        ch.nbins[c] = nbins[c];
        ch.payload[c] = payload ? payload[c] : 0;
        ch.words[c] = words ? words[c] : 0;
    }
    return ch;
}

// host-side checks shared by the three device entry points; `bytes` = size of the packed buffer / container (0: none)
int rans_device_args_ok(int64_t rows, int ld, const int32_t *nbins, int cdf_stride, int steps, const int64_t *payload,
                        const int64_t *words, size_t bytes) {
    if (rows < 0 || ld < 1 || !nbins || !rans_steps_ok(steps)) return SHACIRA_EINVAL;
    if (!symbols_supported(ld)) return SHACIRA_EDTYPE;
    const int64_t nblocks = rans_num_blocks(rows, steps);
    if (nblocks * ld > INT32_MAX || nblocks > INT32_MAX) return SHACIRA_EINVAL;
    for (int c = 0; c < ld; ++c) {
        if (nbins[c] < 0 || nbins[c] > (1 << kRcTotalBits)) return SHACIRA_EINVAL;
        if (nbins[c] < 2) continue;
        if (cdf_stride < nbins[c] + 1) return SHACIRA_EINVAL;
        if (!payload) continue;
        if (!words || payload[c] < 0 || (payload[c] & 3) || words[c] < 0 || words[c] > rows) return SHACIRA_EINVAL;
        const uint64_t end = (uint64_t)payload[c] + (uint64_t)nblocks * kRansBlockHeader + 2 * (uint64_t)words[c];
        if (end > bytes) return SHACIRA_EINVAL;
    }
    return 0;
}

hipError_t rans_encode_launch(const float *latent, int64_t rows, int ld, const int32_t *lo, const int32_t *nbins,
                              const uint32_t *cdf, int cdf_stride, int steps, uint32_t *counts, uint32_t *states,
                              uint16_t *slots, hipStream_t s) {
    const int64_t nblocks = rans_num_blocks(rows, steps);
    const RansChannels ch = rans_channels(ld, lo, nbins, nullptr, nullptr);
    const dim3 grid((uint32_t)nblocks, (uint32_t)ld);
    const size_t lds = rans_cdf_lds(nbins, ld);
    if (lds)
        hipLaunchKernelGGL(rans_encode_kernel<true>, grid, dim3(kRansLanes), lds, s, latent, rows, ld, ch, cdf, cdf_stride,
                           steps, nblocks, counts, states, slots);
    else
        hipLaunchKernelGGL(rans_encode_kernel<false>, grid, dim3(kRansLanes), 0, s, latent, rows, ld, ch, cdf, cdf_stride,
                           steps, nblocks, counts, states, slots);
    return hipGetLastError();
}

hipError_t rans_pack_launch(int64_t rows, int ld, const int32_t *nbins, int steps, const uint32_t *counts,
                            const uint32_t *states, const uint16_t *slots, const int64_t *block_start,
                            const int64_t *payload, const int64_t *words, uint8_t *out, hipStream_t s) {
    const int64_t nblocks = rans_num_blocks(rows, steps);
    const RansChannels ch = rans_channels(ld, nullptr, nbins, payload, words);
    hipLaunchKernelGGL(rans_pack_kernel, dim3((uint32_t)nblocks, (uint32_t)ld), dim3(kSymThreads), 0, s, ch, steps, nblocks,
                       counts, states, slots, block_start, out);
    return hipGetLastError();
}

hipError_t rans_decode_launch(const uint8_t *data, int64_t rows, int ld, const int32_t *lo, const int32_t *nbins,
                              const int64_t *payload, const int64_t *words, const uint32_t *cdf, int cdf_stride,
                              const int64_t *block_start, int steps, float *out, int32_t *error, hipStream_t s) {
    const int64_t nblocks = rans_num_blocks(rows, steps);
    const RansChannels ch = rans_channels(ld, lo, nbins, payload, words);
    const dim3 grid((uint32_t)nblocks, (uint32_t)ld);
    const size_t lds = rans_cdf_lds(nbins, ld);
    if (lds)
        hipLaunchKernelGGL(rans_decode_kernel<true>, grid, dim3(kRansLanes), lds, s, data, ch, cdf, cdf_stride, block_start,
                           steps, nblocks, rows, ld, out, error);
    else
        hipLaunchKernelGGL(rans_decode_kernel<false>, grid, dim3(kRansLanes), 0, s, data, ch, cdf, cdf_stride, block_start,
                           steps, nblocks, rows, ld, out, error);
    return hipGetLastError();
}

}  // namespace shacira
