// nk_query_host.cpp — sequences run against `counts`: nk_query_abundance(_device)
// (kernels: nk_query.hip).  One coverage pass over the query's tiles (the key
// of every window looked up in the table plus the process_sequence delta),
// then the per-record statistics over that coverage.  The query lives in
// buffers of its own (nk_counter::q_*): the retained last input, which the
// on-demand table build and nk_simulate_spikes_auto still need, is not touched.
#include "nk_handle.h"

namespace {

int query_device(nk_counter *c, const uint8_t *d_bases, const uint64_t *d_offs, size_t n_recs,
                 size_t n_bases, uint32_t min_count, uint32_t *d_cov, nk_read_stats *d_stats,
                 hipStream_t s) {
  int rc;
  if (!n_recs) return NK_OK;
  KmerInput in{};
  in.bases = d_bases;
  in.offsets = d_offs;
  in.n_recs = n_recs;
  in.n_bases = n_bases;
  in.n_tiles = n_tiles_for(n_bases, kTile);
  if (in.n_tiles) {
    if ((rc = c->q_trec.ensure(in.n_tiles))) return rc;
    in.tile_rec = c->q_trec.p;
    if (!d_cov) {
      if ((rc = c->q_cov.ensure(n_bases))) return rc;
      d_cov = c->q_cov.p;
    }
    HIPCHK(launch_tile_rec(in, kTile, c->q_trec.p, s));
    HIPCHK(query_coverage(in, (int)c->k, c->canonical, c->w128, table_view(c), delta_args(c), d_cov, s));
  }
  if (!d_stats) return NK_OK;
  if ((rc = c->q_ctr.ensure(2)) || (rc = c->q_mid.ensure(query_mid_cap(n_recs, n_bases))) ||
      (rc = c->q_long.ensure(query_long_cap(n_recs, n_bases))) ||
      (rc = c->q_acc.ensure(query_long_bytes(n_recs, n_bases))))
    return rc;
  HIPCHK(query_stats(d_offs, n_recs, n_bases, (int)c->k, std::max(min_count, 1u), d_cov, d_stats,
                     c->q_mid.p, c->q_long.p, c->q_ctr.p, c->q_acc.p, s));
  return NK_OK;
}

// the stream and the table; what the query cannot answer
int query_ready(nk_counter *c, void *stream, hipStream_t *s) {
  (void)hipSetDevice(c->device);
  *s = pick_stream(c, stream);
  int rc = ensure_table(c, *s);
  if (rc) return rc;
  if (c->exact_built && c->kpn_global)
    return fail(NK_E_UNSUPPORTED,
                "after nk_exact_adopt this rank's table holds only the keys it owns: a query "
                "would have to be routed across the ranks");
  return NK_OK;
}

int check_query(const void *bases, const void *offs, size_t n_recs, size_t n_bases,
                const void *cov, const void *stats) {
  if (!cov && !stats) return fail(NK_E_INVALID, "both outputs are null");
  if (n_recs && (!offs || (n_bases && !bases))) return fail(NK_E_INVALID, "null input with n_recs > 0");
  if (n_bases && !n_recs) return fail(NK_E_INVALID, "bases without records");
  if (n_recs > 0xFFFFFFFFull) return fail(NK_E_INVALID, "more than 2^32 - 1 records");
  return NK_OK;
}

}  // namespace

extern "C" {

int nk_query_abundance_device(nk_counter *c, const uint8_t *d_bases, const uint64_t *d_offs,
                              size_t n_recs, size_t n_bases, uint32_t min_count, uint32_t *d_cov,
                              nk_read_stats *d_stats, void *stream) {
  if (!c) return fail(NK_E_INVALID, "null counter");
  hipStream_t s;
  int rc = query_ready(c, stream, &s);
  if (rc) return rc;
  if ((rc = check_query(d_bases, d_offs, n_recs, n_bases, d_cov, d_stats))) return rc;
  if (n_bases && ((uintptr_t)d_bases & 15))
    return fail(NK_E_INVALID, "device bases must be 16-byte aligned");
  if ((rc = query_device(c, d_bases, d_offs, n_recs, n_bases, min_count, d_cov, d_stats, s)))
    return rc;
  if (!stream) HIPCHK(hipStreamSynchronize(s));
  else record_order(c, s);
  return NK_OK;
}

int nk_query_abundance(nk_counter *c, const uint8_t *bases, const uint64_t *offs, size_t n_recs,
                       uint32_t min_count, uint32_t *cov, nk_read_stats *stats) {
  if (!c) return fail(NK_E_INVALID, "null counter");
  hipStream_t s;
  int rc = query_ready(c, nullptr, &s);
  if (rc) return rc;
  if (!cov && !stats) return fail(NK_E_INVALID, "both outputs are null");
  if (!n_recs) return NK_OK;
  if ((rc = check_offsets(offs, n_recs))) return rc;
  const size_t n_bases = (size_t)offs[n_recs];
  if ((rc = check_query(bases, offs, n_recs, n_bases, cov, stats))) return rc;
  if ((rc = c->q_bases.ensure(n_bases + 16)) || (rc = c->q_offs.ensure(n_recs + 1)) ||
      (rc = c->q_cov.ensure(n_bases)) ||
      (stats && (rc = c->q_stats.ensure(n_recs * sizeof(nk_read_stats)))))
    return rc;
  if (n_bases) HIPCHK(hipMemcpyAsync(c->q_bases.p, bases, n_bases, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(c->q_offs.p, offs, (n_recs + 1) * 8, hipMemcpyHostToDevice, s));
  nk_read_stats *d_stats = stats ? reinterpret_cast<nk_read_stats *>(c->q_stats.p) : nullptr;
  if ((rc = query_device(c, c->q_bases.p, c->q_offs.p, n_recs, n_bases, min_count, c->q_cov.p,
                         d_stats, s)))
    return rc;
  if (cov && n_bases) HIPCHK(hipMemcpyAsync(cov, c->q_cov.p, n_bases * 4, hipMemcpyDeviceToHost, s));
  if (stats)
    HIPCHK(hipMemcpyAsync(stats, d_stats, n_recs * sizeof(nk_read_stats), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return NK_OK;
}

}  // extern "C"
