"""Sequences run against `counts` (neurokmer_amd/csrc/nk_query.hip):
nk_query_abundance / nk_query_abundance_device -- the count of the k-mer
starting at every base of every query record (coverage) and the per-record
statistics (n_kmers, n_present, sum, min, max, khmer's median) -- over every
layout the exact table can have, the process_sequence delta, every key width,
and every path the statistics take by record length.

Expected values need no counter: the table is np.unique over the oracle's
k-mer keys of the table records, a query window's count np.searchsorted into
it (a miss counts 0), the statistics plain numpy with the median
np.sort(c)[c.size // 2].  Bit-exact throughout.
"""
import collections
import contextlib
import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from neurokmer_amd import SpikingKmerCounter, _lib, synth  # noqa: E402
from oracle import cbind  # noqa: E402

NONE = _lib.NK_COV_NONE
WAVE, BLOCK = _lib.NK_QUERY_WAVE_MAX, _lib.NK_QUERY_BLOCK_MAX
ACGT = np.frombuffer(b"ACGT", np.uint8)


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def records(bases, offs):
    return [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(offs.size - 1)]


def arrays(recs):
    """list of byte strings -> (bases, offsets): hand-built, unequal lengths."""
    offs = np.zeros(len(recs) + 1, np.uint64)
    for i, r in enumerate(recs):
        offs[i + 1] = offs[i] + np.uint64(len(r))
    bases = np.frombuffer(b"".join(recs), np.uint8) if recs else np.zeros(0, np.uint8)
    return bases, offs


def table_of(recs, k, canon):
    """(keys ascending, counts) of the records' k-mers."""
    ks = [np.asarray(cbind.kmer_keys(rec, k, canon), np.uint64) for rec in recs]
    ks = [x for x in ks if x.size]
    if not ks:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    u, c = np.unique(np.concatenate(ks), return_counts=True)
    return u.astype(np.uint64), (c & (2**32 - 1)).astype(np.uint32)


def window_counts(rec, k, canon, keys, counts):
    wk = np.asarray(cbind.kmer_keys(rec, k, canon), np.uint64)
    assert wk.size == max(0, len(rec) - k + 1)  # one key per window, in window order
    if not wk.size or not keys.size:
        return np.zeros(wk.size, np.uint32)
    i = np.minimum(np.searchsorted(keys, wk), keys.size - 1)
    return np.where(keys[i] == wk, counts[i], 0).astype(np.uint32)


def stats_of(per_record, min_count=1):
    st = np.zeros(len(per_record), _lib.read_stats_dtype())
    for r, c in enumerate(per_record):
        st["n_kmers"][r] = c.size
        if c.size:
            st["n_present"][r] = int((c >= max(min_count, 1)).sum())
            st["sum"][r] = int(c.astype(np.uint64).sum())
            st["min"][r], st["max"][r] = c.min(), c.max()
            st["median"][r] = np.sort(c)[c.size // 2]
    return st


def expect(qrecs, k, canon, keys, counts, min_count=1, wc=None):
    """(stats, coverage) the query must return."""
    per = [wc(rec) if wc else window_counts(rec, k, canon, keys, counts) for rec in qrecs]
    cov = np.full(sum(len(r) for r in qrecs), NONE, np.uint32)
    at = 0
    for rec, c in zip(qrecs, per):
        cov[at:at + c.size] = c
        at += len(rec)
    return stats_of(per, min_count), cov


def check(g, qrecs, st, cov, min_count=1):
    qb, qo = arrays(qrecs)
    gs, gc = g.abundance_arrays(qb, qo, min_count=min_count, coverage=True)
    assert gs.dtype == st.dtype and gc.dtype == np.uint32
    np.testing.assert_array_equal(gc, cov)
    for f in st.dtype.names:
        np.testing.assert_array_equal(gs[f], st[f], err_msg=f)
    only = g.abundance_arrays(qb, qo, min_count=min_count)  # statistics alone
    assert only.tobytes() == gs.tobytes()
    return gs, gc


def run(bases, offs, k, pool, canon, exact=True, **envkw):
    with env(**envkw):
        g = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, canon, exact_counts=exact)
        g.process_parallel_arrays(bases, offs)
        if not exact:
            g.distinct_kmers()  # builds the table on demand under this environment
        return g


def rand(rng, n):
    return ACGT[rng.integers(0, 4, n)]


def mutated(rng, a, every=40):
    """a with a substitution every `every` bases or so."""
    b = a.copy()
    pos = np.arange(every // 2, b.size, every)
    code = ((b[pos] >> 1) ^ (b[pos] >> 2)) & 3  # A/a 0, C/c 1, G/g 2, T/t 3
    b[pos] = ACGT[(code + 1) % 4]
    return b


MODES = [
    pytest.param(dict(exact=True), id="fused"),
    pytest.param(dict(exact=False), id="standalone"),
    pytest.param(dict(exact=True, NK_EXACT_SORT=1), id="sorted"),
    pytest.param(dict(exact=True, NK_XHASH_MAX=40), id="side"),
    pytest.param(dict(exact=False, NK_XHASH_MAX=40), id="side-standalone"),
    pytest.param(dict(exact=True, NK_XHASH_MAX=40, NK_XSIDE_CAP=1000), id="fallback"),
]
CONFIGS = [(31, 2_000_000, True), (21, 100_003, False)]


@functools.lru_cache(maxsize=None)
def layout_case(k, canon):
    """The table input of test_gpu_enum.py's layouts, and a query over it."""
    bases, offs = synth.make_records(600_000, 5, repeats_per_mb=2000, motif_len=120,
                                     n_rate=0.005, mixed_case=True, seed=41 + k)
    keys, counts = table_of(records(bases, offs), k, canon)
    rng = np.random.default_rng(100 + k)
    rec0 = bases[:int(offs[1])]
    wc0 = window_counts(rec0.tobytes(), k, canon, keys, counts)
    hot = int(np.argmax(wc0))  # inside a planted repeat
    assert wc0[hot] > 1
    lo = max(hot - 20, 0)
    q = [bases[1000:1150], mutated(rng, bases[1000:1150]), rand(rng, 150),
         bases[200_000:200_097], rand(rng, 61),
         # misses, then single-copy windows, then a repeat: min < median < max
         np.concatenate([rand(rng, 150), bases[5000:5300], bases[lo:lo + 110]]),
         bases[300_000:301_200], mutated(rng, bases[300_000:301_200], 97), rand(rng, 700),
         np.concatenate([bases[400_000:406_000], rand(rng, 3000), bases[410_000:413_000]]),
         bases[int(offs[2]) - 70:int(offs[2]) + 90],  # across a table record's end
         rand(rng, k - 1), bases[7:7 + k]]
    qrecs = [x.tobytes() for x in q]
    st, cov = expect(qrecs, k, canon, keys, counts)
    for a in (bases, offs, keys, counts, st, cov):
        a.setflags(write=False)
    return bases, offs, keys, counts, qrecs, st, cov


# ---- 1. layouts ----------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,pool,canon", CONFIGS)
def test_layouts(mode, k, pool, canon):
    bases, offs, keys, counts, qrecs, st, cov = layout_case(k, canon)
    real = cov[cov != NONE]
    assert (real > 0).any() and (real == 0).any() and (real > 1).any()  # hits and misses
    assert ((st["min"] < st["median"]) & (st["median"] < st["max"])).any()
    assert (st["n_kmers"] > BLOCK).any() and (st["n_kmers"] == 0).any()
    g = run(bases, offs, k, pool, canon, **mode)
    check(g, qrecs, st, cov)


# ---- 2. record geometry ----------------------------------------------------------
def test_record_geometry():
    k, pool, canon = CONFIGS[0]
    bases, offs, keys, counts = layout_case(k, canon)[:4]
    g = run(bases, offs, k, pool, canon)
    rng = np.random.default_rng(3)
    lens = [0, 1, k - 1, k, k + 1, 150, 3500,
            WAVE + k - 2, WAVE + k - 1, WAVE + k,        # WAVE - 1, WAVE, WAVE + 1 windows
            0, 0, 0,                                     # empty records in a row
            BLOCK + k - 2, BLOCK + k - 1, BLOCK + k,     # BLOCK - 1, BLOCK, BLOCK + 1 windows
            3, 9000, 2 * 4096 + 500, 0, k - 1, 0, 12]    # ... the last shorter than k
    qrecs, at = [], 20_000
    for i, n in enumerate(lens):  # slices of the table input; every third with substitutions
        a = bases[at:at + n]
        qrecs.append((mutated(rng, a, 55) if i % 3 == 2 and n else a).tobytes())
        at += n + 13
    qb, qo = arrays(qrecs)
    starts, ends = qo[:-1].astype(np.int64), qo[1:].astype(np.int64)
    assert ((starts // 4096 + 1 == ends // 4096) & (ends - starts < 4096)).any()  # crosses one tile edge
    assert (ends // 4096 - starts // 4096 >= 2).any()  # spans three tiles
    st, cov = expect(qrecs, k, canon, keys, counts)
    assert {WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1} <= set(st["n_kmers"].tolist())
    gs, gc = check(g, qrecs, st, cov)
    for s, e in zip(starts, ends):  # the sentinel sits on the last k - 1 bases, nowhere else
        nw = max(0, e - s - k + 1)
        assert (gc[s:s + nw] != NONE).all() and (gc[s + nw:e] == NONE).all()
    assert (gs["_pad"] == 0).all()
    # no records at all
    gs, gc = g.abundance_arrays(np.zeros(0, np.uint8), np.zeros(1, np.uint64), coverage=True)
    assert gs.size == 0 and gc.size == 0
    # one base per record: thousands of records in one tile
    tiny = [bytes([b]) for b in bases[:5000]]
    check(g, tiny + [bases[:100].tobytes()], *expect(tiny + [bases[:100].tobytes()], k, canon, keys, counts))


# ---- 3. median across digits -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deep_case():
    """A poly-A run (one key counted ~70 000 times), a motif planted 400 times,
    single-copy sequence: counts in 1..255, 256..65 535 and past 65 535."""
    k, canon = 31, True
    rng = np.random.default_rng(7)
    motif = rand(rng, 100)
    a = rand(rng, 200_000)
    for i in range(400):
        a[i * 450 + 17:i * 450 + 117] = motif
    b = np.concatenate([rand(rng, 5000), np.full(70_000, ord("A"), np.uint8), rand(rng, 5000)])
    c = rand(rng, 30_001)
    c[::997] = ord("N")
    c[500:900] = np.char.lower(c[500:900].view("S1")).view(np.uint8)
    recs = [a.tobytes(), b.tobytes(), c.tobytes()]
    keys, counts = table_of(recs, k, canon)
    assert counts.max() > 65_535 and ((counts > 255) & (counts < 65_536)).any()
    bases, offs = arrays(recs)
    for x in (bases, offs, keys, counts, motif, a, b, c):
        x.setflags(write=False)
    return bases, offs, keys, counts, motif, a, b, c


def test_median_across_digits():
    bases, offs, keys, counts, motif, a, b, c = deep_case()
    k, canon = 31, True
    rng = np.random.default_rng(8)
    poly = b[5000:75_000]
    q = {  # by statistics class: median in the poly-A key, in the motif, in single-copy sequence
        "wave": [poly[:150], motif, c[1000:1150],
                 np.concatenate([poly[:60], motif, rand(rng, 70)])],
        "block": [poly[:3000], np.tile(motif, 12), c[2000:4000],
                  np.concatenate([poly[:700], np.tile(motif, 9), c[100:500], rand(rng, 300)])],
        "long": [poly[:20_000], np.tile(motif, 150), c[5000:15_000],
                 np.concatenate([poly[:15_000], c[3:15_003], np.tile(motif, 100)]),
                 np.concatenate([np.tile(motif, 250), poly[:9000], rand(rng, 9000)]),
                 np.concatenate([c[:20_000], rand(rng, 14_000)])],
    }
    g = run(bases, offs, k, 2_000_000, canon)
    order = [("long", 0), ("wave", 0), ("block", 0), ("long", 1), ("wave", 1), ("long", 2),
             ("block", 1), ("wave", 2), ("long", 3), ("block", 2), ("long", 4), ("wave", 3),
             ("block", 3), ("long", 5)]
    qrecs = [q[c_][i].tobytes() for c_, i in order]
    st, cov = expect(qrecs, k, canon, keys, counts)
    for cls, (lo, hi) in (("wave", (1, WAVE)), ("block", (WAVE + 1, BLOCK)), ("long", (BLOCK + 1, 2**40))):
        rows = [r for r, (c_, _) in enumerate(order) if c_ == cls]
        assert all(lo <= st["n_kmers"][r] <= hi for r in rows)
        med = st["median"][rows]
        assert ((med >= 1) & (med <= 255)).any(), cls
        assert ((med >= 256) & (med <= 65_535)).any(), cls
        assert (med >= 65_536).any(), cls
    assert (st["n_kmers"] > 2 * 16384).any()  # a long record of several work items
    check(g, qrecs, st, cov)
    g2 = run(bases, offs, k, 2_000_000, canon, NK_EXACT_SORT=1)
    check(g2, qrecs, st, cov)


# ---- 4. min_count ------------------------------------------------------------------
def test_min_count():
    bases, offs, keys, counts, motif, a, b, c = deep_case()
    k, canon = 31, True
    rng = np.random.default_rng(9)
    qrecs = [x.tobytes() for x in (np.concatenate([b[4900:5200], motif, rand(rng, 90)]),
                                   np.concatenate([a[:2000], rand(rng, 500)]),
                                   np.concatenate([b[60_000:76_000], a[:3000]]), rand(rng, 20))]
    g = run(bases, offs, k, 2_000_000, canon)
    base, cov = expect(qrecs, k, canon, keys, counts, 1)
    seen = set()
    for mc in (0, 1, 2, int(counts.max()) + 1):
        st, _ = expect(qrecs, k, canon, keys, counts, mc)
        for f in st.dtype.names:
            if f != "n_present":
                np.testing.assert_array_equal(st[f], base[f])
        check(g, qrecs, st, cov, min_count=mc)
        seen.add(tuple(st["n_present"].tolist()))
    assert len(seen) == 3  # 0 behaves as 1; 2 and max + 1 each differ
    assert not expect(qrecs, k, canon, keys, counts, int(counts.max()) + 1)[0]["n_present"].any()


# ---- 5. the process_sequence delta ----------------------------------------------------
def delta_inputs():
    bases, offs = synth.make_records(120_000, 3, seed=12, repeats_per_mb=1000)
    seqs = (bases[1000:1400].tobytes(), b"ACGTTGCA" * 30, bases[50_000:50_100].tobytes())
    return bases, offs, seqs


def check_delta(g, recs, k, canon, qrecs):
    keys, counts = table_of(recs, k, canon)
    st, cov = expect(qrecs, k, canon, keys, counts)
    gs, gc = check(g, qrecs, st, cov)
    assert (gc[gc != NONE] > 0).any()
    # the same answers as get_counts on the windows' keys
    wk = np.concatenate([np.asarray(cbind.kmer_keys(r, k, canon), np.uint64) for r in qrecs])
    cnt, pres = g.get_counts(wk)
    np.testing.assert_array_equal(cnt, gc[gc != NONE])
    np.testing.assert_array_equal(pres, cnt > 0)


@pytest.mark.parametrize("mode", [dict(), dict(NK_EXACT_SORT=1)], ids=["grouped", "sorted"])
def test_delta_on_a_table(mode):
    bases, offs, seqs = delta_inputs()
    with env(**mode):
        g = SpikingKmerCounter(15, 1.0, 0.95, 2, 1.0, 9_973, True, exact_counts=True)
        g.process_parallel_arrays(bases, offs)
    recs = records(bases, offs)
    for seq in seqs:
        g.process_sequence(seq)
        recs.append(seq)
    rng = np.random.default_rng(5)
    qrecs = list(seqs) + [bases[900:1500].tobytes(), rand(rng, 300).tobytes(), b"ACGTTGCA" * 4,
                          bases[70_000:79_000].tobytes()]
    check_delta(g, recs, 15, True, qrecs)


def test_delta_without_a_table():
    _, _, seqs = delta_inputs()
    g = SpikingKmerCounter(15, 1.0, 0.95, 2, 1.0, 9_973, True, exact_counts=True)
    for seq in seqs:
        g.process_sequence(seq)
    rng = np.random.default_rng(6)
    check_delta(g, list(seqs), 15, True, list(seqs) + [rand(rng, 500).tobytes(), seqs[0][100:300]])


def test_delta_all_t_key():
    """The delta keeps the key ~0 (its empty-slot marker) beside its slots."""
    g = SpikingKmerCounter(32, 1.0, 0.95, 2, 1.0, 3_001, False, exact_counts=True)
    seqs = [b"T" * 40 + b"ACGT" * 20, b"GATTACA" * 9 + b"T" * 33]
    for seq in seqs:
        g.process_sequence(seq)
    keys, counts = table_of(seqs, 32, False)
    assert keys[-1] == 2**64 - 1 and counts[-1] == 11
    qrecs = [b"ACG" + b"T" * 50 + b"GATTACA" * 6, seqs[1], b"T" * 31, b"t" * 32]
    st, cov = expect(qrecs, 32, False, keys, counts)
    assert (cov == 11).sum() >= 19 + 2 + 1
    check_delta(g, seqs, 32, False, qrecs)


# ---- 6. key widths ---------------------------------------------------------------------
@pytest.mark.parametrize("canon", [True, False], ids=["canonical", "forward"])
def test_k40_compat_keys(canon):
    bases, offs = synth.make_records(60_000, 3, repeats_per_mb=3000, motif_len=150, n_rate=0.002,
                                     mixed_case=True, seed=40)
    keys, counts = table_of(records(bases, offs), 40, canon)
    rng = np.random.default_rng(40)
    qrecs = [x.tobytes() for x in (bases[100:400], mutated(rng, bases[100:400]), rand(rng, 200),
                                   bases[19_900:20_100], bases[30_000:39_000], rand(rng, 39),
                                   bases[41_000:41_040], bases[50_000:50_700])]
    st, cov = expect(qrecs, 40, canon, keys, counts)
    real = cov[cov != NONE]
    assert (real > 0).any() and (real == 0).any()
    g = SpikingKmerCounter(40, 1.0, 0.95, 2, 1.0, 50_021, canon, exact_counts=True)
    g.process_parallel_arrays(bases, offs)
    check(g, qrecs, st, cov)


@pytest.mark.parametrize("canon", [True, False], ids=["canonical", "forward"])
@pytest.mark.parametrize("k", [40, 64])
def test_kmer_width_128(k, canon):
    bases, offs = synth.make_records(60_000, 3, repeats_per_mb=3000, motif_len=150, n_rate=0.002,
                                     mixed_case=True, seed=k)
    cnt = collections.Counter()
    for rec in records(bases, offs):
        cnt.update(cbind.kmer_keys128(rec, k, canon))
    assert any(x >> 64 for x in cnt) and max(cnt.values()) >= 2

    def wc(rec):
        ks = cbind.kmer_keys128(rec, k, canon)
        assert len(ks) == max(0, len(rec) - k + 1)
        return np.array([cnt.get(x, 0) for x in ks], np.uint32)

    rng = np.random.default_rng(k)
    qrecs = [x.tobytes() for x in (bases[100:400], mutated(rng, bases[100:400]), rand(rng, 200),
                                   bases[19_900:20_100], bases[30_000:39_000], rand(rng, k - 1),
                                   bases[41_000:41_000 + k], bases[50_000:50_700])]
    st, cov = expect(qrecs, k, canon, None, None, wc=wc)
    real = cov[cov != NONE]
    assert (real > 1).any() and (real == 0).any()
    g = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, 50_021, canon, kmer_width=128, exact_counts=True)
    g.process_parallel_arrays(bases, offs)
    check(g, qrecs, st, cov)


# ---- 7. nothing changes -------------------------------------------------------------------
def snapshot(g):
    keys, cnt = g.counts_arrays()
    return [keys, cnt, g.kmer_per_neuron(), g.currents(), g.spike_counts(),
            np.array(g.top_abundant_neurons(20), np.uint64)]


@pytest.mark.parametrize("exact", [False, True], ids=["lazy", "eager"])
def test_query_changes_nothing(exact):
    k, pool, canon = CONFIGS[1]
    bases, offs, keys, counts, qrecs, st, cov = layout_case(k, canon)
    g = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, canon, exact_counts=exact)
    twin = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, canon, exact_counts=exact)
    for h in (g, twin):
        h.process_parallel_arrays(bases, offs)
    # (lazy: the query is the first call to need the table, built from the retained input)
    check(g, qrecs, st, cov)
    check(g, qrecs[:3], *expect(qrecs[:3], k, canon, keys, counts))
    for x, y in zip(snapshot(g), snapshot(twin)):
        np.testing.assert_array_equal(x, y)
    check(g, qrecs, st, cov)
    for h in (g, twin):  # reads the retained input again (the top rows' uniques)
        h.simulate_spikes_auto()
    np.testing.assert_array_equal(g.spike_counts(), twin.spike_counts())
    assert g.top_abundant_neurons(20) == twin.top_abundant_neurons(20)
    assert g.energy.total_spikes() == twin.energy.total_spikes()
    check(g, qrecs, st, cov)


# ---- 8. device variant -------------------------------------------------------------------
def test_device_variant_and_determinism():
    k, pool, canon = CONFIGS[0]
    bases, offs, keys, counts, qrecs, st, cov = layout_case(k, canon)
    qb, qo = arrays(qrecs)
    n_recs, n_bases = len(qrecs), qb.size
    g, g2 = run(bases, offs, k, pool, canon), run(bases, offs, k, pool, canon)
    hs, hc = check(g, qrecs, st, cov)  # the host variant
    d_b = torch.from_numpy(np.concatenate([qb, np.zeros(16, np.uint8)])).cuda()
    d_o = torch.from_numpy(qo.view(np.int64)).cuda()
    dt = _lib.read_stats_dtype()
    d_cov = torch.full((n_bases,), 77, dtype=torch.int32, device="cuda")
    d_st = torch.full((n_recs * dt.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")
    d_cov2, d_st2 = d_cov.clone(), d_st.clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    args = (d_b.data_ptr(), d_o.data_ptr(), n_recs, n_bases)
    g.abundance_device(*args, d_cov=d_cov.data_ptr(), d_stats=d_st.data_ptr(), stream=s.cuda_stream)
    g.abundance_device(*args, d_stats=d_st2.data_ptr(), stream=s.cuda_stream)  # statistics only
    g.abundance_device(*args, d_cov=d_cov2.data_ptr(), stream=s.cuda_stream)   # coverage only
    s.synchronize()
    for t in (d_cov, d_cov2):
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), hc)
    for t in (d_st, d_st2):
        assert t.cpu().numpy().tobytes() == hs.tobytes()
    # the handle's own stream, waited for
    d_cov.fill_(5)
    torch.cuda.synchronize()
    g.abundance_device(*args, d_cov=d_cov.data_ptr())
    np.testing.assert_array_equal(d_cov.cpu().numpy().view(np.uint32), hc)
    # another handle: identical bytes
    s2, c2 = g2.abundance_arrays(qb, qo, coverage=True)
    assert s2.tobytes() == hs.tobytes() and c2.tobytes() == hc.tobytes()


# ---- 9. empty and unsupported ---------------------------------------------------------------
def test_empty_and_unsupported():
    k, pool, canon = CONFIGS[1]
    bases, offs, keys, counts, qrecs, st, cov = layout_case(k, canon)
    zero_st, zero_cov = expect(qrecs, k, canon, np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert not zero_st["sum"].any() and (zero_st["n_kmers"] == st["n_kmers"]).all()
    for exact in (True, False):
        g = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, canon, exact_counts=exact)
        check(g, qrecs, zero_st, zero_cov)  # fresh: every window counts 0
        g.process_parallel_arrays(bases, offs)
        check(g, qrecs, st, cov)
        g.reset()
        check(g, qrecs, zero_st, zero_cov)
    qb, qo = arrays(qrecs)
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros(16, np.uint8)])).cuda()
    d_o = torch.from_numpy(offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    g = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, canon, exact_counts=False)
    g.process_parallel_device(d_b.data_ptr(), d_o.data_ptr(), offs.size - 1, bases.size)
    with pytest.raises(_lib.NeuroKmerError) as e:  # the caller's device input is not kept
        g.abundance_arrays(qb, qo)
    assert e.value.code == _lib.NK_E_UNSUPPORTED
    g = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, canon, exact_counts=True)
    g.process_parallel_device(d_b.data_ptr(), d_o.data_ptr(), offs.size - 1, bases.size)
    check(g, qrecs, st, cov)
    # both outputs null
    rc = g._L.nk_query_abundance(g._h, qb.ctypes.data, qo.ctypes.data, len(qrecs), 1, None, None)
    assert rc == _lib.NK_E_INVALID
    rc = g._L.nk_query_abundance_device(g._h, d_b.data_ptr(), d_o.data_ptr(), offs.size - 1,
                                        bases.size, 1, None, None, None)
    assert rc == _lib.NK_E_INVALID
    rc = g._L.nk_query_abundance(g._h, None, None, 3, 1, None, np.zeros(120, np.uint8).ctypes.data)
    assert rc == _lib.NK_E_INVALID  # null input with n_recs > 0
    # a rank of a multi-GPU table owns only part of the keys
    n_per, kp, cp = g.exact_partition(1)
    g.exact_adopt(kp, cp, n_per[0])
    with pytest.raises(_lib.NeuroKmerError) as e:
        g.abundance_arrays(qb, qo)
    assert e.value.code == _lib.NK_E_UNSUPPORTED and "rank" in str(e.value)


# ---- 10. CLI ------------------------------------------------------------------------------
def test_cli_query(tmp_path):
    bases, offs = synth.make_records(50_000, 4, repeats_per_mb=4000, motif_len=80, seed=77)
    recs = records(bases, offs)
    fa = tmp_path / "in.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
    rng = np.random.default_rng(77)
    qrecs = [x.tobytes() for x in (bases[100:250], rand(rng, 150), bases[12_000:12_600], rand(rng, 20),
                                   np.concatenate([bases[30_000:30_400], rand(rng, 200)]),
                                   bases[20_000:29_500])]
    qf = tmp_path / "q.fa"
    qf.write_bytes(b"".join(b">q%d\n%s\n" % (i, r) for i, r in enumerate(qrecs)))
    keys, counts = table_of(recs, 21, True)
    base = [_lib.CLI_PATH, "-i", str(fa), "-k", "21", "--pool-size", "4001", "--canonical"]
    plain = subprocess.run(base, capture_output=True, check=True).stdout
    out = tmp_path / "q.tsv"
    for extra, mc in (([], 1), (["--query-min-count", "2"], 2)):
        r = subprocess.run(base + ["--query", str(qf), "--query-out", str(out)] + extra,
                           capture_output=True, check=True)
        assert r.stdout == plain
        st, _ = expect(qrecs, 21, True, keys, counts, mc)
        want = ["\t".join(str(int(x)) for x in (i, s["n_kmers"], s["n_present"], s["min"], s["median"],
                                                s["max"], s["sum"])) for i, s in enumerate(st)]
        assert out.read_text().splitlines() == want
    assert (st["n_present"] > 0).any() and (st["n_kmers"] == 0).any()
    r = subprocess.run(base + ["--query", str(qf)], capture_output=True)
    assert r.returncode != 0 and b"--query-out" in r.stderr
