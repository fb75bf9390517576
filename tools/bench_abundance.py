"""Timing of the read abundance query (nk_query_abundance_device) against the
table of the headline input: config 2 as bench.py generates it (115,000,000
bases in 7 records, k = 31 canonical, pool 2 M), the exact table built
beforehand.

  reads  2,000,000 reads of 150 bases, half of them drawn from the table input
         (the rest fresh random sequence): (a) coverage only, (b) coverage and
         statistics, (c) statistics alone (the coverage goes to the handle's
         scratch), ns per window from (a)
  long   one record of 100,000,000 bases (the table input's first bases): the
         same three, the statistics taking the long path (radix select over HBM)
  old    what the library offered before: get_counts over the same windows'
         keys.  The keys are made on the host by the test oracle (nothing
         exported does that); that time is reported separately and is NOT part
         of the get_counts figure.
each the median of 5 runs after 2 warm-ups (old: --old-runs after 1), beside
the bytes the coverage pass must move (1 B read + 4 B written per position)
at the HBM rates of MI355X (8 TB/s peak, 6.3 TB/s achievable).

Prints one JSON line.  Each step runs in a child process under its own
timeout; the first step that fails ends the run.

    python tools/bench_abundance.py [--bases N] [--reads N] [--long-bases N] [--old-runs R]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

K, POOL, RECS, READ_LEN = 31, 2_000_000, 7, 150
HBM_PEAK_BPS, HBM_REAL_BPS = 8e12, 6.3e12


def timed(fn, runs, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 4), round(min(ts), 4)


def table(bases_n):
    import torch
    from neurokmer_amd import SpikingKmerCounter, synth
    d_b, offs = synth.make_records_torch(bases_n, RECS, seed=synth.SEED, repeats_per_mb=64,
                                         motif_len=200, device="cuda")
    d_o = torch.from_numpy(offs.view("int64")).cuda()
    torch.cuda.synchronize()
    c = SpikingKmerCounter(K, 1.0, 0.95, 2, 1.0, POOL, True, exact_counts=True)
    c.process_parallel_device(d_b.data_ptr(), d_o.data_ptr(), RECS, bases_n)
    return c, d_b, d_o


def make_reads(d_table, table_bases, n_reads):
    """(uint8 tensor of n_reads * 150 + 16 bytes, int64 offsets tensor): the
    first half slices of the table input, the second fresh random sequence."""
    import torch
    from neurokmer_amd import synth
    n_hit = n_reads // 2
    out = torch.zeros(n_reads * READ_LEN + 16, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(20)
    ar = torch.arange(READ_LEN, dtype=torch.int64, device="cuda")
    step = 250_000
    for s in range(0, n_hit, step):
        n = min(step, n_hit - s)
        start = torch.randint(0, table_bases - READ_LEN, (n,), generator=g, device="cuda")
        out[s * READ_LEN:(s + n) * READ_LEN] = d_table[(start[:, None] + ar[None, :]).reshape(-1)]
    n_miss = n_reads - n_hit
    if n_miss:
        synth.random_bases_torch(n_miss * READ_LEN, synth.SEED + 99, 0, out.device,
                                 out=out[n_hit * READ_LEN:n_reads * READ_LEN])
    offs = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * READ_LEN
    torch.cuda.synchronize()
    return out, offs


def three(c, d_b, d_o, n_recs, n_bases, n_windows):
    """coverage only / coverage + statistics / statistics alone."""
    import numpy as np
    import torch
    from neurokmer_amd import _lib
    dt = _lib.read_stats_dtype()
    d_cov = torch.empty(n_bases, dtype=torch.int32, device="cuda")
    d_st = torch.empty(n_recs * dt.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (d_b.data_ptr(), d_o.data_ptr(), n_recs, n_bases)
    out = {"windows": n_windows}
    med, best = timed(lambda: c.abundance_device(*args, d_cov=d_cov.data_ptr()), 5, 2)
    b = 5 * n_bases
    out["coverage"] = {"ms": med, "best_ms": best, "ns_per_window": round(med * 1e6 / n_windows, 4),
                       "bytes": b, "ms_at_8TBs": round(b / HBM_PEAK_BPS * 1e3, 4),
                       "ms_at_6.3TBs": round(b / HBM_REAL_BPS * 1e3, 4)}
    med, best = timed(lambda: c.abundance_device(*args, d_cov=d_cov.data_ptr(),
                                                 d_stats=d_st.data_ptr()), 5, 2)
    out["coverage_and_stats"] = {"ms": med, "best_ms": best}
    both = d_st.cpu().numpy().view(dt).copy()
    d_st.zero_()
    torch.cuda.synchronize()
    med, best = timed(lambda: c.abundance_device(*args, d_stats=d_st.data_ptr()), 5, 2)
    out["stats_alone"] = {"ms": med, "best_ms": best}
    st = d_st.cpu().numpy().view(dt)
    cov = d_cov.cpu().numpy().view(np.uint32)
    real = cov != _lib.NK_COV_NONE
    # consistency at full size (the tests compare bit-exactly at small sizes)
    out["consistent"] = bool(st.tobytes() == both.tobytes() and int(real.sum()) == n_windows
                             and int(st["n_kmers"].sum()) == n_windows
                             and int(st["sum"].sum()) == int(cov[real].astype(np.uint64).sum())
                             and int(st["max"].max()) == int(cov[real].max()))
    out["present_fraction"] = round(float(st["n_present"].sum()) / n_windows, 4)
    return out, st, cov


def step_reads(args):
    import numpy as np
    c, d_table, keep = table(args.bases)
    d_b, d_o = make_reads(d_table, args.bases, args.reads)
    n_bases = args.reads * READ_LEN
    out, st, cov = three(c, d_b, d_o, args.reads, n_bases, args.reads * (READ_LEN - K + 1))
    out["median_of_medians"] = int(np.median(st["median"]))
    # one read's row against its coverage
    c0 = cov[:READ_LEN - K + 1]
    out["consistent"] = bool(out["consistent"] and int(st["median"][0]) == int(np.sort(c0)[c0.size // 2])
                             and int(st["min"][0]) == int(c0.min()))
    return {"reads": out}


def step_long(args):
    import numpy as np
    import torch
    n = min(args.long_bases, args.bases)
    c, d_table, keep = table(args.bases)
    d_o = torch.tensor([0, n], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    out, st, cov = three(c, d_table, d_o, 1, n, n - K + 1)
    part = np.partition(cov[:n - K + 1], (n - K + 1) // 2)
    out["consistent"] = bool(out["consistent"] and int(st["median"][0]) == int(part[(n - K + 1) // 2]))
    out["bases"] = n
    return {"long": out}


def step_old(args):
    import numpy as np
    from oracle import cbind
    c, d_table, keep = table(args.bases)
    d_b, d_o = make_reads(d_table, args.bases, args.reads)
    n_bases = args.reads * READ_LEN
    bases = d_b[:n_bases].cpu().numpy()
    t = time.perf_counter()
    # k <= 32: a window's key depends on its own bases only, so the keys of the
    # concatenation, without the windows that cross a read's end, are the reads' keys
    keys = np.asarray(cbind.kmer_keys(bases.tobytes(), K, True), np.uint64)
    pos = np.arange(keys.size, dtype=np.int64) % READ_LEN
    keys = np.ascontiguousarray(keys[pos <= READ_LEN - K])
    key_ms = (time.perf_counter() - t) * 1e3
    state = {}

    def lookup():
        state["cnt"] = c.get_counts(keys)[0]

    med, best = timed(lookup, args.old_runs, 1)
    d_cov_sum = int(state["cnt"].astype(np.uint64).sum())
    return {"old": {"windows": int(keys.size), "get_counts": {"ms": med, "best_ms": best,
                                                               "runs": args.old_runs},
                    "host_key_making_ms_not_included": round(key_ms, 1),
                    "count_sum": d_cov_sum}}


STEPS = {"reads": (step_reads, 240), "long": (step_long, 240), "old": (step_old, 420)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=115_000_000)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--long-bases", type=int, default=100_000_000)
    ap.add_argument("--old-runs", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="(internal) run one step")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(STEPS[args.step][0](args)), flush=True)
        return 0
    res = {"metric": "read abundance query, config 2 table", "bases": args.bases, "k": K,
           "pool": POOL, "n_reads": args.reads, "read_len": READ_LEN}
    for name, (_, limit) in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--bases", str(args.bases),
               "--reads", str(args.reads), "--long-bases", str(args.long_bases),
               "--old-runs", str(args.old_runs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            res["failed"] = f"{name}: no result within {limit} s"
            break
        if r.returncode != 0:
            res["failed"] = f"{name}: exit {r.returncode}: {r.stderr.strip()[-400:]}"
            break
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
        if res.get(name, {}).get("consistent") is False:
            res["failed"] = f"{name}: the statistics and the coverage disagree at full size"
            break
    if "reads" in res and "old" in res:
        res["speedup_vs_get_counts"] = round(res["old"]["get_counts"]["ms"] / res["reads"]["coverage"]["ms"], 2)
    print(json.dumps(res), flush=True)
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
