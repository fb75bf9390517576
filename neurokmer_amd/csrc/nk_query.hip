// Sequences run against the exact k-mer table (nk_exact.h): the coverage pass
// behind nk_query_abundance(_device) -- the count of the window starting at
// every base, keys made from the staged tile exactly as the table's own keys
// are -- and the per-record statistics over that coverage (n_kmers, n_present,
// sum, min, max and the exact median).
//
// A lookup is a dependent chain of random HBM reads (ent -> the neuron's
// entries -> cnt, or a binary search).  A lane therefore walks kQBatch windows
// in lockstep: every round issues one load per unfinished window before any of
// them is consumed, so a wave keeps up to 64 * kQBatch reads in flight instead
// of one chain after another.
#include "neurokmer.h"
#include "nk_device.h"
#include "nk_exact.h"
#include "nk_tile.h"

namespace nk {

namespace {

constexpr int kQTile = kTile;    // 4096 positions per workgroup
constexpr int kQBlock = kBlock;  // 256 threads
constexpr int kQPer = kQTile / kQBlock;
constexpr int kQBatch = 8;       // windows a lane looks up in lockstep
static_assert(kQPer % kQBatch == 0, "whole batches per thread");

// counts of key[j] (bit j of ok set; the rest 0) in the table plus the delta,
// as k_lookup2 answers them (u32 wrap like AtomicU32)
__device__ __forceinline__ void find_batch(const TableView &t, const DeltaArgs &d,
                                           const uint64_t (&key)[kQBatch], uint32_t ok,
                                           uint32_t (&out)[kQBatch]) {
#pragma unroll
  for (int j = 0; j < kQBatch; ++j) out[j] = 0;
  if (t.n) {
    const uint64_t n0 = t.n[0];
    // lin: a scan of the neuron's entries [lo, hi); else a binary search in
    // the sorted part [lo, hi).  hit: found at lo.
    uint64_t lo[kQBatch], hi[kQBatch];
    uint32_t act = 0, lin = 0, hit = 0;
    if (t.ent) {
      const uint64_t n1 = t.n[1];
      uint64_t e[kQBatch];
#pragma unroll
      for (int j = 0; j < kQBatch; ++j)
        e[j] = (ok >> j) & 1u ? t.ent[fastmod(sip13_u64(key[j]), t.fm)] : 0ull;
#pragma unroll
      for (int j = 0; j < kQBatch; ++j) {
        if (e[j] != kSideEnt) {
          lo[j] = e[j] & ((1ull << 40) - 1);
          hi[j] = lo[j] + (e[j] >> 40);
          lin |= 1u << j;
        } else {
          lo[j] = n1;
          hi[j] = n0;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < kQBatch; ++j) {
        lo[j] = 0;
        hi[j] = n0;
      }
    }
#pragma unroll
    for (int j = 0; j < kQBatch; ++j)
      if (((ok >> j) & 1u) && lo[j] < hi[j]) act |= 1u << j;
    while (act) {
      uint64_t x[kQBatch];
#pragma unroll
      for (int j = 0; j < kQBatch; ++j) {
        x[j] = 0;
        if ((act >> j) & 1u) x[j] = t.uniq[(lin >> j) & 1u ? lo[j] : (lo[j] + hi[j]) >> 1];
      }
#pragma unroll
      for (int j = 0; j < kQBatch; ++j) {
        if (!((act >> j) & 1u)) continue;
        const uint32_t bit = 1u << j;
        if (lin & bit) {
          if (x[j] == key[j]) {
            hit |= bit;
            act &= ~bit;
          } else if (++lo[j] == hi[j]) {
            act &= ~bit;
          }
        } else {
          const uint64_t mid = (lo[j] + hi[j]) >> 1;
          if (x[j] == key[j]) {  // (the sorted part holds a key once)
            lo[j] = mid;
            hit |= bit;
            act &= ~bit;
          } else {
            if (x[j] < key[j]) lo[j] = mid + 1;
            else hi[j] = mid;
            if (lo[j] >= hi[j]) act &= ~bit;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kQBatch; ++j)
      if ((hit >> j) & 1u) out[j] = t.cnt[lo[j]];
  }
  if (d.keys) {  // the process_sequence delta: linear probing from dmix(key)
    uint64_t h[kQBatch];
    uint32_t act = ok;
#pragma unroll
    for (int j = 0; j < kQBatch; ++j) {
      h[j] = dmix(key[j]) & d.mask;
      if (((act >> j) & 1u) && key[j] == kDEmpty) {
        out[j] += (uint32_t)d.meta[0];
        act &= ~(1u << j);
      }
    }
    while (act) {
      unsigned long long cur[kQBatch];
#pragma unroll
      for (int j = 0; j < kQBatch; ++j) {
        cur[j] = kDEmpty;
        if ((act >> j) & 1u) cur[j] = d.keys[h[j]];
      }
#pragma unroll
      for (int j = 0; j < kQBatch; ++j) {
        if (!((act >> j) & 1u)) continue;
        if (cur[j] == kDEmpty) {
          act &= ~(1u << j);
        } else if (cur[j] == key[j]) {
          out[j] += d.vals[h[j]];
          act &= ~(1u << j);
        } else {
          h[j] = (h[j] + 1) & d.mask;
        }
      }
    }
  }
}

// cov[p] = count of the window starting at p, NK_COV_NONE where none starts.
// COMPAT: k > 32, the reference's release-build u64 key straight from the
// record (compat_key), as k_keys_compat makes it; else from the staged tile.
template <bool CANON, bool COMPAT>
__global__ __launch_bounds__(kQBlock) void k_cov(KmerInput in, int k, TableView t, DeltaArgs d,
                                                 uint32_t *__restrict__ cov) {
  __shared__ TileLds<kQTile, !CANON && !COMPAT> L;
  const uint64_t tile = in.tile_base + blockIdx.x;
  const uint64_t T0 = tile * kQTile;
  uint64_t r = 0;
  if constexpr (COMPAT) r = in.tile_rec[blockIdx.x];
  else stage_tile<kQTile, kQBlock, !CANON && !COMPAT>(L, in, tile, k);
#pragma unroll 1
  for (int b = 0; b < kQPer; b += kQBatch) {
    uint64_t key[kQBatch];
    uint32_t ok = 0;
#pragma unroll
    for (int j = 0; j < kQBatch; ++j) {
      const int q = (b + j) * kQBlock + threadIdx.x;
      const uint64_t p = T0 + (uint64_t)q;
      key[j] = 0;
      if (p + (uint64_t)k > in.n_bases) continue;
      if constexpr (COMPAT) {
        while (r + 1 < in.n_recs && in.offsets[r + 1] <= p) ++r;
        const uint64_t s0 = in.offsets[r], e0 = in.offsets[r + 1];
        if (p < s0 || p + (uint64_t)k > e0) continue;
        key[j] = compat_key<CANON>(in.bases, s0, p, k);
      } else {
        if (!window_valid(L, T0, q, k, in.n_bases)) continue;
        key[j] = window_key<kQTile, !CANON, CANON>(L, q, k);
      }
      ok |= 1u << j;
    }
    uint32_t out[kQBatch];
    find_batch(t, d, key, ok, out);
#pragma unroll
    for (int j = 0; j < kQBatch; ++j) {
      const uint64_t p = T0 + (uint64_t)((b + j) * kQBlock + threadIdx.x);
      if (p < in.n_bases) cov[p] = (ok >> j) & 1u ? out[j] : NK_COV_NONE;
    }
  }
}

// NK_KMER_128: window_key128 and the binary search of k_lookup128 (the table is
// sorted, there is no delta), kQBatch windows in lockstep
template <bool CANON>
__global__ __launch_bounds__(kQBlock) void k_cov128(KmerInput in, int k,
                                                    const ulonglong2 *__restrict__ uniq,
                                                    const uint32_t *__restrict__ cnt,
                                                    const unsigned long long *__restrict__ n_uniq,
                                                    uint32_t *__restrict__ cov) {
  __shared__ TileLds<kQTile, !CANON> L;
  const uint64_t tile = in.tile_base + blockIdx.x;
  const uint64_t T0 = tile * kQTile;
  const uint64_t n = n_uniq ? *n_uniq : 0;
  stage_tile<kQTile, kQBlock, !CANON>(L, in, tile, k);
#pragma unroll 1
  for (int b = 0; b < kQPer; b += kQBatch) {
    Key128 key[kQBatch];
    uint64_t lo[kQBatch], hi[kQBatch];
    uint32_t ok = 0, act = 0, hit = 0;
#pragma unroll
    for (int j = 0; j < kQBatch; ++j) {
      const int q = (b + j) * kQBlock + threadIdx.x;
      key[j] = Key128{0, 0};
      lo[j] = 0;
      hi[j] = n;
      if (T0 + (uint64_t)q + (uint64_t)k > in.n_bases) continue;
      if (!window_valid(L, T0, q, k, in.n_bases)) continue;
      key[j] = window_key128<kQTile, !CANON, CANON>(L, q, k);
      ok |= 1u << j;
      if (n) act |= 1u << j;
    }
    while (act) {
      ulonglong2 x[kQBatch];
#pragma unroll
      for (int j = 0; j < kQBatch; ++j) {
        x[j] = make_ulonglong2(0, 0);
        if ((act >> j) & 1u) x[j] = uniq[(lo[j] + hi[j]) >> 1];
      }
#pragma unroll
      for (int j = 0; j < kQBatch; ++j) {
        if (!((act >> j) & 1u)) continue;
        const uint32_t bit = 1u << j;
        const uint64_t mid = (lo[j] + hi[j]) >> 1;
        const Key128 xx{x[j].x, x[j].y};  // (lo, hi) words of the u128
        if (xx.lo == key[j].lo && xx.hi == key[j].hi) {
          lo[j] = mid;
          hit |= bit;
          act &= ~bit;
        } else {
          if (key128_less(xx, key[j])) lo[j] = mid + 1;
          else hi[j] = mid;
          if (lo[j] >= hi[j]) act &= ~bit;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kQBatch; ++j) {
      const uint64_t p = T0 + (uint64_t)((b + j) * kQBlock + threadIdx.x);
      const uint32_t v = (hit >> j) & 1u ? cnt[lo[j]] : 0u;
      if (p < in.n_bases) cov[p] = (ok >> j) & 1u ? v : NK_COV_NONE;
    }
  }
}

// ---- per-record statistics -------------------------------------------------------
// Windows of record r: cov[s, s + nw), s = offsets[r], nw = max(0, len - k + 1)
// (the geometry, never the NK_COV_NONE sentinel).  Three classes by nw:
//   nw <= kQWaveMax    one wave, the counts in registers
//   nw <= kQBlockMax   one workgroup, the counts in LDS
//   longer             many workgroups per record, the counts re-read from HBM
// The first two find the median bit by bit from the top bit of the record's
// max: with the bits above `bit` decided (prefix), c0 = the counts that agree
// with the prefix and have bit 0; the rank m stays below c0 or moves past it.
// The long class does the same a byte at a time over a 256-bin histogram.
constexpr int kQWavePer = NK_QUERY_WAVE_MAX / 64;
constexpr int kQWaves = kQBlock / 64;
constexpr int kQChunk = 16384;  // windows per work item of the long class
static_assert(NK_QUERY_WAVE_MAX % 64 == 0 && NK_QUERY_BLOCK_MAX % kQBlock == 0, "class limits");

struct QAgg {
  unsigned long long sum;
  uint32_t np, mn, mx;
};
__device__ __forceinline__ void agg_add(QAgg &a, uint32_t v, uint32_t min_count) {
  a.sum += v;
  a.np += v >= min_count ? 1u : 0u;
  a.mn = v < a.mn ? v : a.mn;
  a.mx = v > a.mx ? v : a.mx;
}
__device__ __forceinline__ void agg_wave(QAgg &a) {
  for (int o = 32; o > 0; o >>= 1) {
    a.sum += __shfl_xor(a.sum, o, 64);
    a.np += __shfl_xor(a.np, o, 64);
    const uint32_t mn = __shfl_xor(a.mn, o, 64), mx = __shfl_xor(a.mx, o, 64);
    a.mn = mn < a.mn ? mn : a.mn;
    a.mx = mx > a.mx ? mx : a.mx;
  }
}
// every thread gets the workgroup's aggregate (two barriers)
__device__ __forceinline__ void agg_block(QAgg &a, QAgg *s_a) {
  agg_wave(a);
  if ((threadIdx.x & 63) == 0) s_a[threadIdx.x >> 6] = a;
  __syncthreads();
  a = s_a[0];
  for (int w = 1; w < kQWaves; ++w) {
    a.sum += s_a[w].sum;
    a.np += s_a[w].np;
    a.mn = s_a[w].mn < a.mn ? s_a[w].mn : a.mn;
    a.mx = s_a[w].mx > a.mx ? s_a[w].mx : a.mx;
  }
  __syncthreads();
}
__device__ __forceinline__ uint32_t sum_block(uint32_t v, uint32_t *s_c) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = v;
  __syncthreads();
  v = 0;
  for (int w = 0; w < kQWaves; ++w) v += s_c[w];
  __syncthreads();
  return v;
}
__device__ __forceinline__ void put_stats(nk_read_stats *st, uint64_t nw, const QAgg &a,
                                          uint32_t median) {
  nk_read_stats o;
  o.n_kmers = nw;
  o.n_present = a.np;
  o.sum = a.sum;
  o.min = nw ? a.mn : 0u;
  o.max = a.mx;
  o.median = nw ? median : 0u;
  o._pad = 0;
  *st = o;
}
__device__ __forceinline__ uint64_t windows_of(const uint64_t *offs, uint64_t r, int k,
                                               uint64_t *s) {
  *s = offs[r];
  const uint64_t len = offs[r + 1] - *s;
  return len >= (uint64_t)k ? len - (uint64_t)k + 1 : 0;
}

// a wave per record; longer records are listed for the two kernels below
// (ctr[0] / ctr[1]: one atomic per such record)
__global__ __launch_bounds__(kQBlock) void k_stats_wave(const uint64_t *__restrict__ offs,
                                                        uint64_t n_recs, int k, uint32_t min_count,
                                                        const uint32_t *__restrict__ cov,
                                                        nk_read_stats *__restrict__ st,
                                                        uint32_t *__restrict__ mid_list,
                                                        uint32_t *__restrict__ long_list,
                                                        unsigned long long *__restrict__ ctr) {
  const int lane = threadIdx.x & 63;
  const uint64_t r = (uint64_t)blockIdx.x * kQWaves + (threadIdx.x >> 6);
  if (r >= n_recs) return;
  uint64_t s;
  const uint64_t nw = windows_of(offs, r, k, &s);
  if (nw > NK_QUERY_WAVE_MAX) {
    if (lane == 0) {
      if (nw <= NK_QUERY_BLOCK_MAX) mid_list[atomicAdd(&ctr[0], 1ull)] = (uint32_t)r;
      else long_list[atomicAdd(&ctr[1], 1ull)] = (uint32_t)r;
    }
    return;
  }
  uint32_t v[kQWavePer], has = 0;
  QAgg a{0, 0, ~0u, 0};
#pragma unroll
  for (int i = 0; i < kQWavePer; ++i) {
    const uint32_t idx = i * 64 + lane;
    v[i] = 0;
    if (idx < nw) {
      v[i] = cov[s + idx];
      has |= 1u << i;
      agg_add(a, v[i], min_count);
    }
  }
  agg_wave(a);
  uint32_t m = (uint32_t)(nw >> 1), prefix = 0;
  if (nw)
    for (int bit = 31 - __clz((int)(a.mx | 1u)); bit >= 0; --bit) {
      uint32_t c0 = 0;
#pragma unroll
      for (int i = 0; i < kQWavePer; ++i)
        c0 += (uint32_t)__popcll(__ballot(((has >> i) & 1u) && ((v[i] ^ prefix) >> bit) == 0));
      if (m >= c0) {
        m -= c0;
        prefix |= 1u << bit;
      }
    }
  if (lane == 0) put_stats(st + r, nw, a, prefix);
}

// a workgroup per listed record, its counts in LDS
__global__ __launch_bounds__(kQBlock) void k_stats_block(const uint64_t *__restrict__ offs, int k,
                                                         uint32_t min_count,
                                                         const uint32_t *__restrict__ cov,
                                                         nk_read_stats *__restrict__ st,
                                                         const uint32_t *__restrict__ mid_list,
                                                         const unsigned long long *__restrict__ ctr) {
  __shared__ uint32_t sv[NK_QUERY_BLOCK_MAX];
  __shared__ QAgg s_a[kQWaves];
  __shared__ uint32_t s_c[kQWaves];
  const uint64_t n_mid = ctr[0];
  for (uint64_t i = blockIdx.x; i < n_mid; i += gridDim.x) {
    const uint64_t r = mid_list[i];
    uint64_t s;
    const uint64_t nw64 = windows_of(offs, r, k, &s);
    const uint32_t nw = (uint32_t)(nw64 < NK_QUERY_BLOCK_MAX ? nw64 : NK_QUERY_BLOCK_MAX);
    QAgg a{0, 0, ~0u, 0};
    for (uint32_t idx = threadIdx.x; idx < nw; idx += kQBlock) {
      const uint32_t v = cov[s + idx];
      sv[idx] = v;
      agg_add(a, v, min_count);
    }
    agg_block(a, s_a);  // (its barriers also publish sv)
    uint32_t m = nw >> 1, prefix = 0;
    for (int bit = 31 - __clz((int)(a.mx | 1u)); bit >= 0; --bit) {
      uint32_t c0 = 0;
      for (uint32_t idx = threadIdx.x; idx < nw; idx += kQBlock)
        c0 += ((sv[idx] ^ prefix) >> bit) == 0 ? 1u : 0u;
      c0 = sum_block(c0, s_c);
      if (m >= c0) {
        m -= c0;
        prefix |= 1u << bit;
      }
    }
    if (threadIdx.x == 0) put_stats(st + r, nw, a, prefix);
    __syncthreads();
  }
}

// The long class.  Per listed record an accumulator in HBM; each workgroup
// adds its chunks' partial results with a few atomics per (record, pass),
// never one per window.
struct QLong {
  unsigned long long sum, np, rank;
  uint32_t nmn, mx, prefix, _pad;  // nmn = ~min (grows from 0 by atomicMax)
  unsigned long long hist[256];
};

__global__ __launch_bounds__(kQBlock) void k_long_init(QLong *__restrict__ acc,
                                                       const unsigned long long *__restrict__ ctr) {
  const uint64_t n_words = ctr[1] * (sizeof(QLong) / 8);
  unsigned long long *w = reinterpret_cast<unsigned long long *>(acc);
  for (uint64_t i = (uint64_t)blockIdx.x * kQBlock + threadIdx.x; i < n_words;
       i += (uint64_t)gridDim.x * kQBlock)
    w[i] = 0;
}

__global__ __launch_bounds__(kQBlock) void k_long_stats(const uint64_t *__restrict__ offs, int k,
                                                        uint32_t min_count,
                                                        const uint32_t *__restrict__ cov,
                                                        const uint32_t *__restrict__ long_list,
                                                        const unsigned long long *__restrict__ ctr,
                                                        QLong *__restrict__ acc) {
  __shared__ QAgg s_a[kQWaves];
  const uint64_t n_long = ctr[1];
  for (uint64_t i = 0; i < n_long; ++i) {
    uint64_t s;
    const uint64_t nw = windows_of(offs, long_list[i], k, &s);
    const uint64_t n_chunks = (nw + kQChunk - 1) / kQChunk;
    if (blockIdx.x >= n_chunks) continue;  // (uniform)
    QAgg a{0, 0, ~0u, 0};
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
      const uint64_t b = c * kQChunk, e = b + kQChunk < nw ? b + kQChunk : nw;
      for (uint64_t idx = b + threadIdx.x; idx < e; idx += kQBlock) agg_add(a, cov[s + idx], min_count);
    }
    agg_block(a, s_a);
    if (threadIdx.x == 0) {
      atomicAdd(&acc[i].sum, a.sum);
      atomicAdd(&acc[i].np, (unsigned long long)a.np);
      atomicMax(&acc[i].nmn, ~a.mn);
      atomicMax(&acc[i].mx, a.mx);
    }
  }
}

// A pass is skipped for a record whose max has no bit at or above the byte:
// every count's digit is 0 there and neither the prefix nor the rank moves.
__device__ __forceinline__ bool long_skip(uint32_t mx, int byte) {
  return byte > 0 && (mx >> (8 * byte)) == 0;
}

// hist[digit `byte` of v] += 1 over the counts that agree with the prefix
// above that byte.  Within a wave, equal digits of the first two distinct
// values are added once (most counts of a long record are equal: same-address
// LDS atomics serialise); the workgroup's LDS histogram is flushed with one
// global atomic per non-zero bin.
__global__ __launch_bounds__(kQBlock) void k_long_hist(const uint64_t *__restrict__ offs, int k,
                                                       const uint32_t *__restrict__ cov,
                                                       const uint32_t *__restrict__ long_list,
                                                       const unsigned long long *__restrict__ ctr,
                                                       QLong *__restrict__ acc, int byte) {
  __shared__ uint32_t sh[256];
  const uint64_t n_long = ctr[1];
  const int lane = threadIdx.x & 63;
  for (uint64_t i = 0; i < n_long; ++i) {
    uint64_t s;
    const uint64_t nw = windows_of(offs, long_list[i], k, &s);
    const uint64_t n_chunks = (nw + kQChunk - 1) / kQChunk;
    if (blockIdx.x >= n_chunks || long_skip(acc[i].mx, byte)) continue;  // (uniform)
    const uint32_t prefix = acc[i].prefix;
    sh[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
      const uint64_t b = c * kQChunk, e = b + kQChunk < nw ? b + kQChunk : nw;
      for (uint64_t i0 = b; i0 < e; i0 += kQBlock) {  // (uniform trip count: ballots below)
        const uint64_t idx = i0 + threadIdx.x;
        const uint32_t v = idx < e ? cov[s + idx] : 0u;
        bool todo = idx < e && (byte == 3 || ((v ^ prefix) >> (8 * (byte + 1))) == 0);
        const uint32_t dg = (v >> (8 * byte)) & 255u;
        for (int round = 0; round < 2; ++round) {
          const uint64_t m = __ballot(todo);
          if (!m) break;
          const int leader = __ffsll((long long)m) - 1;
          const uint32_t ld = __shfl(dg, leader, 64);
          const uint64_t same = __ballot(todo && dg == ld);
          if (lane == leader) atomicAdd(&sh[ld], (uint32_t)__popcll(same));
          if (dg == ld) todo = false;
        }
        if (todo) atomicAdd(&sh[dg], 1u);
      }
    }
    __syncthreads();
    if (sh[threadIdx.x]) atomicAdd(&acc[i].hist[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
    __syncthreads();
  }
}

// the digit holding the rank: prefix and rank move on, the histogram is
// zeroed for the next pass; the last pass (byte 0) writes the record's row
__global__ __launch_bounds__(256) void k_long_pick(const uint64_t *__restrict__ offs, int k,
                                                   const uint32_t *__restrict__ long_list,
                                                   const unsigned long long *__restrict__ ctr,
                                                   QLong *__restrict__ acc, int byte,
                                                   nk_read_stats *__restrict__ st) {
  __shared__ unsigned long long sc[256];
  const uint64_t n_long = ctr[1];
  for (uint64_t i = blockIdx.x; i < n_long; i += gridDim.x) {
    const uint32_t mx = acc[i].mx;
    if (long_skip(mx, byte)) continue;  // (uniform)
    uint64_t s;
    const uint64_t nw = windows_of(offs, long_list[i], k, &s);
    // the first pass that runs for this record starts from rank nw / 2
    const bool first = byte == 3 || (mx >> (8 * (byte + 1))) == 0;
    const unsigned long long rank = first ? nw >> 1 : acc[i].rank;
    const uint32_t prefix = acc[i].prefix;
    const unsigned long long h = acc[i].hist[threadIdx.x];
    sc[threadIdx.x] = h;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan
      const unsigned long long y = threadIdx.x >= (uint32_t)o ? sc[threadIdx.x - o] : 0ull;
      __syncthreads();
      sc[threadIdx.x] += y;
      __syncthreads();
    }
    const unsigned long long incl = sc[threadIdx.x], excl = incl - h;
    acc[i].hist[threadIdx.x] = 0;
    if (excl <= rank && rank < incl) {  // exactly one thread: the counts sum to more than rank
      const uint32_t p = prefix | (uint32_t)threadIdx.x << (8 * byte);
      acc[i].prefix = p;
      acc[i].rank = rank - excl;
      if (byte == 0) {
        const QAgg a{acc[i].sum, 0, ~acc[i].nmn, mx};
        put_stats(st + long_list[i], nw, a, p);
        st[long_list[i]].n_present = acc[i].np;
      }
    }
    __syncthreads();
  }
}

}  // namespace

hipError_t query_coverage(const KmerInput &in, int k, int canonical, bool w128, const TableView &t,
                          const DeltaArgs &d, uint32_t *cov, hipStream_t s) {
  if (!in.n_tiles) return hipSuccess;
  if (in.n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const dim3 g((unsigned)in.n_tiles), b(kQBlock);
  if (w128) {
    const ulonglong2 *u = reinterpret_cast<const ulonglong2 *>(t.uniq);
    if (canonical) hipLaunchKernelGGL(k_cov128<true>, g, b, 0, s, in, k, u, t.cnt, t.n, cov);
    else hipLaunchKernelGGL(k_cov128<false>, g, b, 0, s, in, k, u, t.cnt, t.n, cov);
  } else if (k <= 32) {
    if (canonical) hipLaunchKernelGGL((k_cov<true, false>), g, b, 0, s, in, k, t, d, cov);
    else hipLaunchKernelGGL((k_cov<false, false>), g, b, 0, s, in, k, t, d, cov);
  } else {
    if (canonical) hipLaunchKernelGGL((k_cov<true, true>), g, b, 0, s, in, k, t, d, cov);
    else hipLaunchKernelGGL((k_cov<false, true>), g, b, 0, s, in, k, t, d, cov);
  }
  return hipGetLastError();
}

size_t query_mid_cap(size_t n_recs, size_t n_bases) {
  const size_t m = n_bases / (NK_QUERY_WAVE_MAX + 1) + 1;
  return m < n_recs ? m : n_recs;
}
size_t query_long_cap(size_t n_recs, size_t n_bases) {
  const size_t m = n_bases / (NK_QUERY_BLOCK_MAX + 1) + 1;
  return m < n_recs ? m : n_recs;
}
size_t query_long_bytes(size_t n_recs, size_t n_bases) {
  return query_long_cap(n_recs, n_bases) * sizeof(QLong);
}

hipError_t query_stats(const uint64_t *offs, size_t n_recs, size_t n_bases, int k,
                       uint32_t min_count, const uint32_t *cov, nk_read_stats *st,
                       uint32_t *mid_list, uint32_t *long_list, unsigned long long *ctr,
                       void *long_acc, hipStream_t s) {
  if (!n_recs) return hipSuccess;
  if (n_recs > 0xFFFFFFFFull) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(ctr, 0, 16, s);
  if (e != hipSuccess) return e;
  const unsigned gw = (unsigned)((n_recs + kQWaves - 1) / kQWaves);
  hipLaunchKernelGGL(k_stats_wave, dim3(gw), dim3(kQBlock), 0, s, offs, (uint64_t)n_recs, k,
                     min_count, cov, st, mid_list, long_list, ctr);
  const size_t mid = query_mid_cap(n_recs, n_bases), lng = query_long_cap(n_recs, n_bases);
  // (a record of either list has more than NK_QUERY_WAVE_MAX windows)
  if (n_bases <= (size_t)NK_QUERY_WAVE_MAX) return hipGetLastError();
  hipLaunchKernelGGL(k_stats_block, dim3((unsigned)(mid < 2048 ? mid : 2048)), dim3(kQBlock), 0, s,
                     offs, k, min_count, cov, st, mid_list, ctr);
  if (n_bases <= (size_t)NK_QUERY_BLOCK_MAX) return hipGetLastError();
  QLong *acc = static_cast<QLong *>(long_acc);
  const unsigned gl = (unsigned)(lng < 256 ? lng : 256);
  // 4 workgroups per CU: enough loads in flight for a streaming read
  const uint64_t chunks = (n_bases + kQChunk - 1) / kQChunk;
  const unsigned gc = (unsigned)(chunks < 1024 ? chunks : 1024);
  hipLaunchKernelGGL(k_long_init, dim3(gl), dim3(kQBlock), 0, s, acc, ctr);
  hipLaunchKernelGGL(k_long_stats, dim3(gc), dim3(kQBlock), 0, s, offs, k, min_count, cov,
                     long_list, ctr, acc);
  for (int byte = 3; byte >= 0; --byte) {
    hipLaunchKernelGGL(k_long_hist, dim3(gc), dim3(kQBlock), 0, s, offs, k, cov, long_list, ctr, acc,
                       byte);
    hipLaunchKernelGGL(k_long_pick, dim3(gl), dim3(256), 0, s, offs, k, long_list, ctr, acc, byte, st);
  }
  return hipGetLastError();
}

}  // namespace nk
