"""Timing of the table enumeration (nk_export_counts_device, nk_count_spectrum)
on the headline input: config 2 as bench.py generates it (115,000,000 bases in
7 records, k = 31 canonical, pool 2 M), the exact table built beforehand.

  (a) spectrum(10001)
  (b) counts_device() with the default range
  (c) counts_device(min_count=2)
each the median of 5 runs after 2 warm-ups, beside its algorithmic bytes
(entries x bytes read + written) at 8 TB/s, and the only route to the same
answers without these calls: exact_partition(1), a copy of the pairs to the
host, np.bincount / np.argsort there (the host sort takes seconds per run:
--host-runs of it, default 3 after 1 warm-up).

Prints one JSON line.  Each step runs in a child process under its own
timeout; the first step that fails ends the run.

    python tools/bench_enum.py [--bases N] [--host-runs R]
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

K, POOL, RECS = 31, 2_000_000, 7
HBM_BPS = 8e12


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
    return c, (d_b, d_o)


def step_new(args):
    import numpy as np
    c, keep = table(args.bases)
    n = c.distinct_kmers()
    out = {"distinct_kmers": n}
    med, best = timed(lambda: c.spectrum(10001), 5, 2)
    b = 4 * n
    out["spectrum_10001"] = {"ms": med, "best_ms": best, "bytes": b,
                             "roofline_ms": round(b / HBM_BPS * 1e3, 4)}
    med, best = timed(lambda: c.counts_device(), 5, 2)
    b = 24 * n  # 12 B read + 12 B written per pair
    out["counts_device_all"] = {"ms": med, "best_ms": best, "bytes": b,
                                "roofline_ms": round(b / HBM_BPS * 1e3, 4)}
    n2 = c.counts_device(2)[2]
    med, best = timed(lambda: c.counts_device(2), 5, 2)
    b = 12 * n + 12 * n2
    out["counts_device_min2"] = {"ms": med, "best_ms": best, "pairs": n2, "bytes": b,
                                 "roofline_ms": round(b / HBM_BPS * 1e3, 4)}
    h = c.spectrum(10001)
    out["spectrum_head"] = [int(x) for x in h[:6]]
    # consistency at full size (the tests compare bit-exactly at small sizes)
    keys, counts = c.counts_arrays()
    ok = (keys.size == n and int(h.sum()) == n and n2 == n - int(h[1])
          and bool((keys[1:] > keys[:-1]).all())
          and bool((np.bincount(np.minimum(counts, 10000), minlength=10001) == h).all()))
    out["consistent"] = ok
    return out


def step_old(args):
    import numpy as np
    from neurokmer_amd import _lib
    c, keep = table(args.bases)
    state = {}

    def fetch(with_keys):
        cnt, kp, cp = c.exact_partition(1)
        n = cnt[0]
        counts = np.empty(n, np.uint32)
        _lib.copy_from_device(counts.ctypes.data, cp, 4 * n)
        state["counts"] = counts
        if with_keys:
            keys = np.empty(n, np.uint64)
            _lib.copy_from_device(keys.ctypes.data, kp, 8 * n)
            state["keys"] = keys

    def spectrum():
        fetch(False)
        state["hist"] = np.bincount(np.minimum(state["counts"], 10000), minlength=10001)

    def sort_pairs():
        o = np.argsort(state["keys"], kind="stable")
        state["sorted"] = (state["keys"][o], state["counts"][o])

    out = {}
    med, best = timed(spectrum, 5, 2)
    out["old_spectrum"] = {"ms": med, "best_ms": best}
    med, best = timed(lambda: fetch(True), 5, 2)
    out["old_fetch_pairs"] = {"ms": med, "best_ms": best}
    smed, sbest = timed(sort_pairs, args.host_runs, 1)
    out["old_host_argsort"] = {"ms": smed, "best_ms": sbest, "runs": args.host_runs}
    out["old_export"] = {"ms": round(med + smed, 4)}
    out["old_pairs"] = int(state["keys"].size)  # what exact_partition(1) returned
    out["old_spectrum_head"] = [int(x) for x in state["hist"][:6]]
    return out


STEPS = {"new": (step_new, 240), "old": (step_old, 420)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=115_000_000)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="(internal) run one step")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(STEPS[args.step][0](args)), flush=True)
        return 0
    res = {"metric": "table enumeration, config 2 input", "bases": args.bases, "k": K, "pool": POOL}
    for name, (_, limit) in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--bases", str(args.bases),
               "--host-runs", str(args.host_runs)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            res["failed"] = f"{name}: no result within {limit} s"
            break
        if r.returncode != 0:
            res["failed"] = f"{name}: exit {r.returncode}: {r.stderr.strip()[-400:]}"
            break
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
        if res.get("consistent") is False:
            res["failed"] = "the export and the spectrum disagree at full size"
            break
    print(json.dumps(res), flush=True)
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
