// Enumeration of the exact k-mer table (nk_exact.h): the order-preserving
// range filter behind nk_export_counts(_device) and the abundance spectrum
// behind nk_count_spectrum.  Both are streaming passes over (key, count)
// arrays that already sit in HBM; the sort and merge of the grouped layout and
// of the process_sequence delta are exact_merge_pairs (nk_exact.hip).
#include "nk_device.h"
#include "nk_exact.h"

namespace nk {

namespace {

constexpr int kEnBlock = 256;
constexpr int kEnPer = kEnumTile / kEnBlock;  // 16 entries per thread
constexpr int kEnWaves = kEnBlock / 64;
static_assert(kEnPer * kEnWaves == 64, "one wave scans the per-(round, wave) counts");

__device__ __forceinline__ uint64_t en_count(const unsigned long long *n, uint64_t max_n) {
  if (!n) return max_n;
  const uint64_t v = *n;
  return v < max_n ? v : max_n;  // never past what the host sized the buffers for
}

// pass 1: survivors of each workgroup's tile (4 B per entry read)
__global__ __launch_bounds__(kEnBlock) void k_enum_count(const uint32_t *__restrict__ cnt,
                                                         const unsigned long long *__restrict__ n_ptr,
                                                         uint64_t max_n, uint32_t lo, uint32_t hi,
                                                         unsigned long long *__restrict__ wg) {
  __shared__ uint32_t s_w[kEnWaves];
  const uint64_t n = en_count(n_ptr, max_n);
  const uint64_t base = (uint64_t)blockIdx.x * kEnumTile;
  uint32_t k = 0;
#pragma unroll
  for (int j = 0; j < kEnPer; ++j) {
    const uint64_t i = base + (uint64_t)j * kEnBlock + threadIdx.x;
    const uint32_t c = i < n ? cnt[i] : 0u;
    k += (i < n && c >= lo && c <= hi) ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) k += __shfl_down(k, o, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = k;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kEnWaves; ++w) t += s_w[w];
    wg[blockIdx.x] = t;
  }
}

// the workgroup counts -> exclusive offsets (from *at, null: 0), in place; one
// workgroup: thread t owns a run of ceil(G / 256) consecutive counts
__global__ __launch_bounds__(kEnBlock) void k_enum_scan(unsigned long long *__restrict__ wg, uint64_t G,
                                                        const unsigned long long *__restrict__ at,
                                                        unsigned long long *__restrict__ n_out) {
  __shared__ unsigned long long s[kEnBlock];
  const uint64_t per = (G + kEnBlock - 1) / kEnBlock;
  const uint64_t b = (uint64_t)threadIdx.x * per, e = b + per < G ? b + per : G;
  unsigned long long sum = 0;
  for (uint64_t i = b; i < e; ++i) sum += wg[i];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < kEnBlock; o <<= 1) {  // inclusive scan of the run sums
    const unsigned long long y = threadIdx.x >= (uint32_t)o ? s[threadIdx.x - o] : 0ull;
    __syncthreads();
    s[threadIdx.x] += y;
    __syncthreads();
  }
  const unsigned long long base = at ? *at : 0ull;
  unsigned long long run = base + s[threadIdx.x] - sum;
  for (uint64_t i = b; i < e; ++i) {
    const unsigned long long c = wg[i];
    wg[i] = run;
    run += c;
  }
  if (threadIdx.x == kEnBlock - 1) *n_out = base + s[kEnBlock - 1];
}

// pass 2: every survivor to its scanned offset, in entry order (q = j * 256 +
// tid within the tile): the wave ballot + mbcnt give the rank inside a wave's
// round, one wave scans the 64 (round, wave) totals.  K = u64, or 16 B for the
// (lo, hi) pairs of NK_KMER_128 (one 16-byte load and store per key).
template <typename K>
__global__ __launch_bounds__(kEnBlock) void k_enum_write(const K *__restrict__ keys,
                                                         const uint32_t *__restrict__ cnt,
                                                         const unsigned long long *__restrict__ n_ptr,
                                                         uint64_t max_n, uint32_t lo, uint32_t hi,
                                                         K *__restrict__ out_keys,
                                                         uint32_t *__restrict__ out_cnt,
                                                         const unsigned long long *__restrict__ wg) {
  __shared__ uint32_t pre[kEnPer * kEnWaves];
  const uint64_t n = en_count(n_ptr, max_n);
  const uint64_t base = (uint64_t)blockIdx.x * kEnumTile;
  if (base >= n) return;  // (uniform: the whole workgroup)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t cv[kEnPer], rank[kEnPer], ok = 0;
#pragma unroll
  for (int j = 0; j < kEnPer; ++j) {
    const uint64_t i = base + (uint64_t)j * kEnBlock + threadIdx.x;
    cv[j] = i < n ? cnt[i] : 0u;
    const bool keep = i < n && cv[j] >= lo && cv[j] <= hi;
    const uint64_t m = __ballot(keep);
    rank[j] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (keep) ok |= 1u << j;
    if (lane == 0) pre[j * kEnWaves + w] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const uint32_t c = pre[threadIdx.x];
    uint32_t incl = c;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(incl, o, 64);
      if (lane >= o) incl += y;
    }
    pre[threadIdx.x] = incl - c;
  }
  __syncthreads();
  const unsigned long long o0 = wg[blockIdx.x];
#pragma unroll
  for (int j = 0; j < kEnPer; ++j)
    if ((ok >> j) & 1u) {
      const uint64_t i = base + (uint64_t)j * kEnBlock + threadIdx.x;
      const unsigned long long at = o0 + pre[j * kEnWaves + w] + rank[j];
      out_keys[at] = keys[i];
      out_cnt[at] = cv[j];
    }
}

// the delta's all-ones key (kept in meta[0], nk_exact.hip delta_add) appended
// to the gathered pairs
__global__ void k_enum_delta_ones(const unsigned long long *__restrict__ meta,
                                  uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_cnt,
                                  unsigned long long *__restrict__ n) {
  if (blockIdx.x || threadIdx.x) return;
  const uint32_t v = (uint32_t)meta[0];
  if (!v) return;
  const unsigned long long at = *n;
  out_keys[at] = ~0ull;
  out_cnt[at] = v;
  *n = at + 1;
}

// hist[j] += entries with count j (j < n_bins - 1), hist[n_bins - 1] += the
// rest; count 0 (a hole of the grouped layout) is no entry.  Counts 2 ..
// kSpecLds - 1 go to the workgroup's LDS histogram, flushed with one global
// atomic per non-zero bin; count 1 (most k-mers of real data) and the high bin
// stay in registers and are added once per wave: same-address LDS atomics
// serialise.  Counts in [kSpecLds, n_bins - 1) are rare: global atomics.
__global__ __launch_bounds__(kEnBlock) void k_spectrum(const uint32_t *__restrict__ cnt,
                                                       const unsigned long long *__restrict__ n_ptr,
                                                       uint64_t max_n, uint32_t n_bins,
                                                       unsigned long long *__restrict__ hist) {
  __shared__ uint32_t sh[kSpecLds];
  for (int i = threadIdx.x; i < kSpecLds; i += kEnBlock) sh[i] = 0;
  __syncthreads();
  const uint64_t n = en_count(n_ptr, max_n);
  const uint32_t top = n_bins - 1;
  uint32_t ones = 0, high = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kEnBlock + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * kEnBlock) {
    const uint32_t c = cnt[i];
    if (c == 0) continue;
    if (c >= top) ++high;
    else if (c == 1) ++ones;
    else if (c < (uint32_t)kSpecLds) atomicAdd(&sh[c], 1u);
    else atomicAdd(&hist[c], 1ull);
  }
  for (int o = 32; o > 0; o >>= 1) {
    ones += __shfl_down(ones, o, 64);
    high += __shfl_down(high, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (ones) atomicAdd(&sh[1], ones);
    if (high) atomicAdd(&hist[top], (unsigned long long)high);
  }
  __syncthreads();
  const uint32_t end = top < (uint32_t)kSpecLds ? top : (uint32_t)kSpecLds;
  for (uint32_t i = threadIdx.x; i < end; i += kEnBlock)
    if (sh[i]) atomicAdd(&hist[i], (unsigned long long)sh[i]);
}

}  // namespace

hipError_t enum_filter_count(const uint32_t *cnt, const unsigned long long *n, size_t max_n,
                             uint32_t lo, uint32_t hi, unsigned long long *wg,
                             const unsigned long long *at, unsigned long long *n_out,
                             hipStream_t s) {
  const uint64_t G = enum_groups(max_n);
  if (G > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (G) hipLaunchKernelGGL(k_enum_count, dim3((unsigned)G), dim3(kEnBlock), 0, s, cnt, n,
                            (uint64_t)max_n, lo, hi, wg);
  hipLaunchKernelGGL(k_enum_scan, dim3(1), dim3(kEnBlock), 0, s, wg, G, at, n_out);
  return hipGetLastError();
}

hipError_t enum_filter_write(const uint64_t *keys, const uint32_t *cnt, const unsigned long long *n,
                             size_t max_n, int wpk, uint32_t lo, uint32_t hi, uint64_t *out_keys,
                             uint32_t *out_cnt, const unsigned long long *wg, hipStream_t s) {
  const uint64_t G = enum_groups(max_n);
  if (!G) return hipSuccess;
  if (G > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (wpk == 2)
    hipLaunchKernelGGL(k_enum_write<ulonglong2>, dim3((unsigned)G), dim3(kEnBlock), 0, s,
                       reinterpret_cast<const ulonglong2 *>(keys), cnt, n, (uint64_t)max_n, lo, hi,
                       reinterpret_cast<ulonglong2 *>(out_keys), out_cnt, wg);
  else
    hipLaunchKernelGGL(k_enum_write<uint64_t>, dim3((unsigned)G), dim3(kEnBlock), 0, s, keys, cnt,
                       n, (uint64_t)max_n, lo, hi, out_keys, out_cnt, wg);
  return hipGetLastError();
}

hipError_t enum_delta_ones(const unsigned long long *meta, uint64_t *out_keys, uint32_t *out_cnt,
                           unsigned long long *n, hipStream_t s) {
  hipLaunchKernelGGL(k_enum_delta_ones, dim3(1), dim3(64), 0, s, meta, out_keys, out_cnt, n);
  return hipGetLastError();
}

hipError_t enum_spectrum(const uint32_t *cnt, const unsigned long long *n, size_t max_n,
                         uint32_t n_bins, unsigned long long *hist, hipStream_t s) {
  if (n_bins < 2) return hipErrorInvalidValue;
  if (!max_n) return hipSuccess;
  // 32 KiB of LDS per workgroup: 5 workgroups (20 waves) per CU, 256 CUs
  uint64_t g = (max_n + 8 * kEnBlock - 1) / (8 * kEnBlock);
  if (g > 1280) g = 1280;
  hipLaunchKernelGGL(k_spectrum, dim3((unsigned)g), dim3(kEnBlock), 0, s, cnt, n, (uint64_t)max_n,
                     n_bins, hist);
  return hipGetLastError();
}

}  // namespace nk
