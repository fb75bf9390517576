// nk_enum_host.cpp — the whole of `counts` (the reference's counts.iter(),
// src/python.rs:30-36): nk_export_counts(_device) and nk_count_spectrum over
// the exact table plus the process_sequence delta (kernels: nk_enum.hip).
//
//   sorted table, no delta    the table is the merged view already
//   grouped table / a delta   gather (the table's non-hole entries, then the
//                             delta's used slots and its ~0 key: two runs of
//                             the filter with the range 1..2^32-1), then
//                             exact_merge_pairs: sort + counts of equal keys summed
//   range filter              count pass; when every entry survives the merged
//                             view itself is returned, else the write pass
//   spectrum                  straight over the table's counts when there is no
//                             delta (holes have count 0), else over the merged counts
#include "nk_handle.h"

namespace {

// (key, count) arrays holding every key of `counts` once
struct EnumSrc {
  const uint64_t *keys = nullptr;
  const uint32_t *cnt = nullptr;
  const unsigned long long *n = nullptr;  // device: entries
  uint64_t max_n = 0;                      // host bound of *n (0: empty)
  bool merged = false;                     // en_k2 / en_c2 (else the table's own arrays)
};

// need_sorted: keys ascending and no holes between them (the export); else any
// order, zero-count holes allowed (the spectrum)
int enum_source(nk_counter *c, bool need_sorted, hipStream_t s, EnumSrc &src) {
  int rc;
  unsigned long long base_n = 0;
  if (c->exact_built) {
    HIPCHK(hipMemcpyAsync(&base_n, c->x_n.p + 1, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  const DeltaArgs d = delta_args(c);
  const bool live = d.keys != nullptr;
  if (!live && (!c->x_grouped || !need_sorted)) {
    if (base_n) {
      src.keys = c->x_uniq.p;
      src.cnt = c->x_cnt.p;
      src.n = c->x_n.p + 1;
      src.max_n = base_n;
    }
    return NK_OK;
  }
  const uint64_t d_n = live ? c->d_cap : 0;
  const uint64_t bound = base_n + d_n + 1;
  if ((rc = c->en_n.ensure(8)) || (rc = c->en_k0.ensure(bound)) || (rc = c->en_c0.ensure(bound)) ||
      (rc = c->en_wg.ensure(enum_groups(std::max<uint64_t>(base_n, d_n)) + 1)))
    return rc;
  HIPCHK(hipMemsetAsync(c->en_n.p, 0, 64, s));
  if (base_n) {
    HIPCHK(enum_filter_count(c->x_cnt.p, c->x_n.p + 1, base_n, 1u, ~0u, c->en_wg.p, nullptr,
                             c->en_n.p, s));
    HIPCHK(enum_filter_write(c->x_uniq.p, c->x_cnt.p, c->x_n.p + 1, base_n, 1, 1u, ~0u,
                             c->en_k0.p, c->en_c0.p, c->en_wg.p, s));
  }
  if (live) {
    // a used slot has a non-zero value, a free one 0 (delta_clear)
    HIPCHK(enum_filter_count(d.vals, nullptr, d_n, 1u, ~0u, c->en_wg.p, c->en_n.p, c->en_n.p + 1, s));
    HIPCHK(enum_filter_write((const uint64_t *)d.keys, d.vals, nullptr, d_n, 1, 1u, ~0u, c->en_k0.p,
                             c->en_c0.p, c->en_wg.p, s));
    HIPCHK(enum_delta_ones(d.meta, c->en_k0.p, c->en_c0.p, c->en_n.p + 1, s));
  } else {
    HIPCHK(hipMemcpyAsync(c->en_n.p + 1, c->en_n.p, 8, hipMemcpyDeviceToDevice, s));
  }
  unsigned long long n_g = 0;
  HIPCHK(hipMemcpyAsync(&n_g, c->en_n.p + 1, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (!n_g) return NK_OK;
  if (n_g > bound) return fail(NK_E_DEVICE, "enumeration gathered %llu pairs into %llu", n_g,
                               (unsigned long long)bound);
  const int end_bit = (int)std::min<uint64_t>(64, 2 * c->k);  // (k > 32: u64 compat keys)
  if ((rc = c->en_k1.ensure(n_g)) || (rc = c->en_c1.ensure(n_g)) || (rc = c->en_k2.ensure(n_g)) ||
      (rc = c->en_c2.ensure(n_g)) || (rc = c->en_tmp.ensure(exact_merge_temp_bytes(n_g, end_bit))))
    return rc;
  HIPCHK(exact_merge_pairs(c->en_k0.p, c->en_c0.p, n_g, end_bit, c->en_k1.p, c->en_c1.p,
                           c->en_k2.p, c->en_c2.p, c->en_n.p + 2, c->en_tmp.p, c->en_tmp.n, s));
  src.keys = c->en_k2.p;
  src.cnt = c->en_c2.p;
  src.n = c->en_n.p + 2;
  src.max_n = n_g;
  src.merged = true;
  return NK_OK;
}

// the stream and the table for an enumeration call
int enum_ready(nk_counter *c, void *stream, hipStream_t *s) {
  (void)hipSetDevice(c->device);
  *s = pick_stream(c, stream);
  return ensure_table(c, *s);
}

}  // namespace

extern "C" {

int nk_export_counts_device(nk_counter *c, uint32_t min_count, uint32_t max_count,
                            const uint64_t **d_keys, const uint32_t **d_counts, size_t *n,
                            void *stream) {
  if (!c) return fail(NK_E_INVALID, "null counter");
  if (!d_keys || !d_counts || !n) return fail(NK_E_INVALID, "null argument");
  if (min_count > max_count)
    return fail(NK_E_INVALID, "min_count (%u) > max_count (%u)", min_count, max_count);
  hipStream_t s;
  int rc = enum_ready(c, stream, &s);
  if (rc) return rc;
  const int w = c->w128 ? 2 : 1;
  const uint32_t lo = std::max(min_count, 1u);  // a zero count is no entry
  if ((rc = c->en_n.ensure(8)) || (rc = c->en_k0.ensure(2)) || (rc = c->en_c0.ensure(1))) return rc;
  EnumSrc src;
  if (max_count >= lo && (rc = enum_source(c, true, s, src))) return rc;
  *d_keys = c->en_k0.p;
  *d_counts = c->en_c0.p;
  *n = 0;
  if (!src.max_n) return NK_OK;
  if ((rc = c->en_wg.ensure(enum_groups(src.max_n) + 1))) return rc;
  HIPCHK(enum_filter_count(src.cnt, src.n, src.max_n, lo, max_count, c->en_wg.p, nullptr,
                           c->en_n.p + 3, s));
  unsigned long long h[2] = {0, 0};  // merged keys, survivors
  HIPCHK(hipMemcpyAsync(h, c->en_n.p + 2, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const unsigned long long n_src = src.merged ? h[0] : src.max_n;
  if (h[1] == n_src) {  // nothing to drop: the merged view is the answer
    *d_keys = src.keys;
    *d_counts = src.cnt;
    *n = (size_t)n_src;
    return NK_OK;
  }
  if (h[1]) {
    if ((rc = c->en_k0.ensure((uint64_t)w * h[1])) || (rc = c->en_c0.ensure(h[1]))) return rc;
    HIPCHK(enum_filter_write(src.keys, src.cnt, src.n, src.max_n, w, lo, max_count, c->en_k0.p,
                             c->en_c0.p, c->en_wg.p, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  *d_keys = c->en_k0.p;
  *d_counts = c->en_c0.p;
  *n = (size_t)h[1];
  return NK_OK;
}

long nk_export_counts(nk_counter *c, uint32_t min_count, uint32_t max_count, uint64_t *keys,
                      uint32_t *counts, size_t cap) {
  if (!c) return fail(NK_E_INVALID, "null counter");
  if (cap && (!keys || !counts)) return fail(NK_E_INVALID, "null output with cap > 0");
  const uint64_t *dk = nullptr;
  const uint32_t *dc = nullptr;
  size_t total = 0;
  int rc = nk_export_counts_device(c, min_count, max_count, &dk, &dc, &total, nullptr);
  if (rc) return rc;
  const size_t m = std::min(total, cap);
  if (m) {
    HIPCHK(hipMemcpy(keys, dk, m * (c->w128 ? 16 : 8), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(counts, dc, m * 4, hipMemcpyDeviceToHost));
  }
  return (long)total;
}

int nk_count_spectrum(nk_counter *c, uint64_t *hist, size_t n_bins) {
  if (n_bins < 2 || n_bins > ((size_t)1 << 20))
    return fail(NK_E_INVALID, "n_bins (%zu) must be in 2..2^20", n_bins);
  if (!c) return fail(NK_E_INVALID, "null counter");
  if (!hist) return fail(NK_E_INVALID, "null output");
  hipStream_t s;
  int rc = enum_ready(c, nullptr, &s);
  if (rc) return rc;
  EnumSrc src;
  if ((rc = enum_source(c, false, s, src))) return rc;
  if (!src.max_n) {
    memset(hist, 0, n_bins * 8);
    return NK_OK;
  }
  if ((rc = c->en_hist.ensure(n_bins))) return rc;
  HIPCHK(hipMemsetAsync(c->en_hist.p, 0, n_bins * 8, s));
  HIPCHK(enum_spectrum(src.cnt, src.n, src.max_n, (uint32_t)n_bins, c->en_hist.p, s));
  HIPCHK(hipMemcpyAsync(hist, c->en_hist.p, n_bins * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return NK_OK;
}

}  // extern "C"
