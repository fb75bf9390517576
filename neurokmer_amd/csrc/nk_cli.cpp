// nk_cli.cpp — `neurokmer` CLI, the MI355X drop-in for the reference binary
// (src/main.rs:9-77).  Same flags (-i/--input, -k/--k [31], --pool-size
// [1000000], --canonical, --streaming), same LIF constants (threshold 1.0,
// leak 0.95, refractory 2, spike_cost 1.0: src/main.rs:36-37) and the same
// result block on stdout (src/main.rs:49-74).  Uses only the C ABI.
#include <charconv>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "neurokmer.h"
#include "nk_fastx.h"

// Rust `{}` for f64: shortest round-trip digits in positional notation.
static std::string rust_f64(double x) {
  if (x != x) return "NaN";
  if (x == 1.0 / 0.0) return "inf";
  if (x == -1.0 / 0.0) return "-inf";
  char buf[512];
  auto res = std::to_chars(buf, buf + sizeof buf, x, std::chars_format::fixed);
  std::string s(buf, res.ptr);
  return s;
}

static void usage() {
  fprintf(stderr,
          "Neuromorphic k-mer counting with fixed-size spiking neuron pool\n\n"
          "Usage: neurokmer [OPTIONS] --input <INPUT>\n\n"
          "Options:\n"
          "  -i, --input <INPUT>\n"
          "  -k, --k <K>                  [default: 31]\n"
          "      --pool-size <POOL_SIZE>  [default: 1000000]\n"
          "      --canonical\n"
          "      --streaming\n"
          "      --device <N>             HIP device ordinal [default: 0]\n"
          "      --spectrum <FILE>        Write the abundance spectrum: 'count n_kmers' lines\n"
          "      --spectrum-max <N>       Largest count with a line of its own [default: 10000]\n"
          "      --counts <FILE>          Write every k-mer as 'KMER<TAB>count', in key order (k <= 32)\n"
          "      --min-count <N>          Smallest count --counts writes [default: 1]\n"
          "      --query <FILE>           FASTA/FASTQ records to run against the k-mer table\n"
          "      --query-out <FILE>       Per query record: 'index n_kmers n_present min median max sum' (tabs)\n"
          "      --query-min-count <N>    Smallest count of a present k-mer [default: 1]\n"
          "  -h, --help                   Print help\n");
}

static bool parse_u64(const char *s, unsigned long long &out) {
  char *end = nullptr;
  if (!s || !*s || *s == '-') return false;
  out = strtoull(s, &end, 10);
  return end && *end == 0;
}

// --spectrum: one 'count n_kmers' line per non-empty bin, ascending (the last
// bin holds every count >= spectrum_max + 1, as jellyfish histo's high bin)
static int write_spectrum(nk_counter *c, const std::string &path, size_t n_bins) {
  std::vector<uint64_t> hist(n_bins);
  if (nk_count_spectrum(c, hist.data(), n_bins)) {
    fprintf(stderr, "Error: %s\n", nk_last_error());
    return 1;
  }
  FILE *f = fopen(path.c_str(), "w");
  if (!f) {
    fprintf(stderr, "Error: cannot write %s\n", path.c_str());
    return 1;
  }
  for (size_t j = 1; j < n_bins; ++j)
    if (hist[j]) fprintf(f, "%zu %llu\n", j, (unsigned long long)hist[j]);
  return fclose(f) ? 1 : 0;
}

// --counts: 'KMER<TAB>count' per key in key order; the k-mer is the 2-bit key
// decoded, first base in the highest bits (A C G T = 0 1 2 3)
static int write_counts(nk_counter *c, const std::string &path, unsigned k, uint32_t min_count) {
  long total = nk_export_counts(c, min_count, UINT32_MAX, nullptr, nullptr, 0);
  if (total < 0) {
    fprintf(stderr, "Error: %s\n", nk_last_error());
    return 1;
  }
  std::vector<uint64_t> keys((size_t)total);
  std::vector<uint32_t> cnt((size_t)total);
  if (total && nk_export_counts(c, min_count, UINT32_MAX, keys.data(), cnt.data(), (size_t)total) < 0) {
    fprintf(stderr, "Error: %s\n", nk_last_error());
    return 1;
  }
  FILE *f = fopen(path.c_str(), "w");
  if (!f) {
    fprintf(stderr, "Error: cannot write %s\n", path.c_str());
    return 1;
  }
  std::string kmer(k, 'A');
  for (long i = 0; i < total; ++i) {
    for (unsigned j = 0; j < k; ++j) kmer[j] = "ACGT"[(keys[i] >> (2 * (k - 1 - j))) & 3];
    fprintf(f, "%s\t%u\n", kmer.c_str(), cnt[i]);
  }
  return fclose(f) ? 1 : 0;
}

// --query / --query-out: the query file's records (the host reader, plain or
// gzip) against the table of the run; one line per record, in file order
static int write_query(nk_counter *c, const std::string &query, const std::string &path,
                       uint32_t min_count) {
  std::vector<uint8_t> bases;
  std::vector<uint64_t> offs;
  std::string err;
  if (nk::read_fastx_all(query.c_str(), bases, offs, err)) {
    fprintf(stderr, "Error: %s\n", err.c_str());
    return 1;
  }
  const size_t n = offs.size() - 1;
  std::vector<nk_read_stats> st(n);
  if (nk_query_abundance(c, bases.data(), offs.data(), n, min_count, nullptr, st.data())) {
    fprintf(stderr, "Error: %s\n", nk_last_error());
    return 1;
  }
  FILE *f = fopen(path.c_str(), "w");
  if (!f) {
    fprintf(stderr, "Error: cannot write %s\n", path.c_str());
    return 1;
  }
  for (size_t i = 0; i < n; ++i)
    fprintf(f, "%zu\t%llu\t%llu\t%u\t%u\t%u\t%llu\n", i, (unsigned long long)st[i].n_kmers,
            (unsigned long long)st[i].n_present, st[i].min, st[i].median, st[i].max,
            (unsigned long long)st[i].sum);
  return fclose(f) ? 1 : 0;
}

int main(int argc, char **argv) {
  std::string input, spectrum_path, counts_path, query_path, query_out;
  unsigned long long k = 31, pool = 1000000, device = 0, spectrum_max = 10000, min_count = 1;
  unsigned long long query_min = 1;
  bool canonical = false, streaming = false, have_input = false;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto val = [&](const char *name) -> const char * {
      size_t eq = a.find('=');
      if (eq != std::string::npos) return argv[i] + eq + 1;
      if (i + 1 >= argc) {
        fprintf(stderr, "error: a value is required for '%s'\n", name);
        exit(2);
      }
      return argv[++i];
    };
    auto is = [&](const char *opt) {
      return a == opt || a.rfind(std::string(opt) + "=", 0) == 0;
    };
    if (a == "-h" || a == "--help") {
      usage();
      return 0;
    } else if (a == "-i" || is("--input")) {
      input = val("--input <INPUT>");
      have_input = true;
    } else if (a == "-k" || is("--k")) {
      if (!parse_u64(val("--k <K>"), k)) { fprintf(stderr, "error: invalid value for '--k <K>'\n"); return 2; }
    } else if (is("--pool-size")) {
      if (!parse_u64(val("--pool-size <POOL_SIZE>"), pool)) { fprintf(stderr, "error: invalid value for '--pool-size <POOL_SIZE>'\n"); return 2; }
    } else if (a == "--canonical") {
      canonical = true;
    } else if (a == "--streaming") {
      streaming = true;
    } else if (is("--device")) {
      if (!parse_u64(val("--device <N>"), device)) { fprintf(stderr, "error: invalid value for '--device <N>'\n"); return 2; }
    } else if (is("--spectrum-max")) {
      if (!parse_u64(val("--spectrum-max <N>"), spectrum_max) || spectrum_max > (1ull << 20) - 2) { fprintf(stderr, "error: invalid value for '--spectrum-max <N>'\n"); return 2; }
    } else if (is("--spectrum")) {
      spectrum_path = val("--spectrum <FILE>");
    } else if (is("--min-count")) {
      if (!parse_u64(val("--min-count <N>"), min_count) || min_count > 0xFFFFFFFFull) { fprintf(stderr, "error: invalid value for '--min-count <N>'\n"); return 2; }
    } else if (is("--counts")) {
      counts_path = val("--counts <FILE>");
    } else if (is("--query-out")) {
      query_out = val("--query-out <FILE>");
    } else if (is("--query-min-count")) {
      if (!parse_u64(val("--query-min-count <N>"), query_min) || query_min > 0xFFFFFFFFull) { fprintf(stderr, "error: invalid value for '--query-min-count <N>'\n"); return 2; }
    } else if (is("--query")) {
      query_path = val("--query <FILE>");
    } else {
      fprintf(stderr, "error: unexpected argument '%s' found\n", a.c_str());
      usage();
      return 2;
    }
  }
  if (!have_input) {
    fprintf(stderr, "error: the following required arguments were not provided:\n  --input <INPUT>\n");
    usage();
    return 2;
  }
  if (!counts_path.empty() && k > 32) {
    fprintf(stderr, "error: --counts decodes 2-bit keys (k <= 32); the keys of k = %llu are not k-mers\n", k);
    return 2;
  }
  if (query_path.empty() != query_out.empty()) {
    fprintf(stderr, "error: --query <FILE> and --query-out <FILE> go together\n");
    usage();
    return 2;
  }
  fprintf(stderr, "[INFO neurokmer] Starting NeuroKmer on %s (k=%llu, pool_size=%llu, canonical=%s, streaming=%s)\n",
          input.c_str(), k, pool, canonical ? "true" : "false", streaming ? "true" : "false");

  nk_opts opts;
  nk_opts_default(&opts);
  opts.device = (int32_t)device;
  nk_counter *c = nk_new((size_t)k, 1.0f, 0.95f, 2, 1.0, (size_t)pool, canonical ? 1 : 0, &opts);
  if (!c) {
    fprintf(stderr, "Error: %s\n", nk_last_error());
    return 1;
  }
  int rc;
  if (streaming) {
    printf("Starting streaming for: %s\n", input.c_str());
    rc = nk_process_file_streaming(c, input.c_str());
  } else {
    // stream_sequences(input).collect() + process_parallel (src/main.rs:40-46),
    // parsed on the device (nk_process_file_parallel)
    rc = nk_process_file_parallel(c, input.c_str());
    if (!rc) {
      std::vector<uint64_t> cur(nk_pool_size(c));
      unsigned long long tot = 0;
      if (!cur.empty() && nk_copy_currents(c, cur.data(), cur.size()) == 0)
        for (uint64_t x : cur) tot += x;
      printf("  In-memory total current: %llu\n", tot);  // src/spiking_hash.rs:184
    }
  }
  if (rc) {
    fprintf(stderr, "Error: %s\n", nk_last_error());
    nk_free(c);
    return 1;
  }
  printf("\n=== Top 20 Abundant Neuron Groups (Highest Spike Rates) ===\n");
  std::vector<nk_top_row> top(20);
  long n = nk_top_abundant_neurons(c, 20, top.data());
  if (n < 0) {
    fprintf(stderr, "Error: %s\n", nk_last_error());
    nk_free(c);
    return 1;
  }
  if (n == 0) {
    printf("No spikes fired (empty file or too small k)\n");
  } else {
    for (long i = 0; i < n; ++i)
      printf("%3ld: Neuron %6llu \xe2\x86\x92 %8llu spikes (%u unique k-mers colliding)\n", i + 1,
             (unsigned long long)top[i].idx, (unsigned long long)top[i].spikes, top[i].uniques);
  }
  fprintf(stderr, "[INFO neurokmer] Processing complete - total spikes: %llu, energy: %s\n",
          (unsigned long long)nk_total_spikes(c), rust_f64(nk_energy_used(c)).c_str());
  printf("\nTotal spikes fired: %llu\n", (unsigned long long)nk_total_spikes(c));
  printf("Simulated energy used: %s\n", rust_f64(nk_energy_used(c)).c_str());
  printf("Neuron pool size used: %llu\n", pool);
  printf("Streaming mode: %s\n", streaming ? "true" : "false");
  int out_rc = 0;
  if (!spectrum_path.empty()) out_rc = write_spectrum(c, spectrum_path, (size_t)spectrum_max + 2);
  if (!out_rc && !counts_path.empty()) out_rc = write_counts(c, counts_path, (unsigned)k, (uint32_t)min_count);
  if (!out_rc && !query_path.empty()) out_rc = write_query(c, query_path, query_out, (uint32_t)query_min);
  nk_free(c);
  return out_rc;
}
