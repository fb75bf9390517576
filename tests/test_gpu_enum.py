"""Enumeration of `counts` (neurokmer_amd/csrc/nk_enum.hip): the export of every
(key, count) pair in key order (nk_export_counts / _device) and the abundance
spectrum (nk_count_spectrum), over every layout the exact table can have
(sorted, grouped with holes and a side part, the key 0 and ~0 cases, the
process_sequence delta, 128-bit keys).

The reference exposes the same data as `counts.iter()` (src/python.rs:30-36,
unordered).  Expected values need no counter: np.unique over the k-mer keys of
every record is the export, np.bincount of those counts (clipped at
n_bins - 1) the spectrum.  Bit-exact throughout.
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

U32_MAX = 2**32 - 1


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


def expected(recs, k, canon):
    """(keys ascending, counts) of the records' k-mers."""
    ks = [cbind.kmer_keys(rec, k, canon) for rec in recs]
    ks = [np.asarray(x, np.uint64) for x in ks if len(x)]
    if not ks:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    u, c = np.unique(np.concatenate(ks), return_counts=True)
    return u.astype(np.uint64), (c & U32_MAX).astype(np.uint32)


def expected_spectrum(counts, n_bins):
    h = np.bincount(np.minimum(counts.astype(np.int64), n_bins - 1), minlength=n_bins)
    return h.astype(np.uint64)


def check_all(g, keys, counts, bins=(64, 5000)):
    gk, gc = g.counts_arrays()
    assert gk.dtype == np.uint64 and gc.dtype == np.uint32
    np.testing.assert_array_equal(gk, keys)
    np.testing.assert_array_equal(gc, counts)
    for nb in bins:
        h = g.spectrum(nb)
        assert h.dtype == np.uint64 and h.size == nb and h[0] == 0
        np.testing.assert_array_equal(h, expected_spectrum(counts, nb))
        assert int(h.sum()) == g.distinct_kmers() == keys.size


def run(bases, offs, k, pool, canon, exact=True, **envkw):
    with env(**envkw):
        g = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, canon, exact_counts=exact)
        g.process_parallel_arrays(bases, offs)
        if not exact:
            g.distinct_kmers()  # builds the table on demand under this environment
        return g


MODES = [
    pytest.param(dict(exact=True), id="fused"),
    pytest.param(dict(exact=False), id="standalone"),
    pytest.param(dict(exact=True, NK_EXACT_SORT=1), id="sorted"),
    pytest.param(dict(exact=True, NK_XHASH_MAX=40), id="side"),
    pytest.param(dict(exact=False, NK_XHASH_MAX=40), id="side-standalone"),
    pytest.param(dict(exact=True, NK_XHASH_MAX=40, NK_XSIDE_CAP=1000), id="fallback"),
]
CONFIGS = [(31, 2_000_000, True), (21, 100_003, False), (40, 50_021, True)]


@functools.lru_cache(maxsize=None)
def layout_case(k, canon):
    bases, offs = synth.make_records(600_000, 5, repeats_per_mb=2000, motif_len=120,
                                     n_rate=0.005, mixed_case=True, seed=41 + k)
    keys, counts = expected(records(bases, offs), k, canon)
    for a in (bases, offs, keys, counts):
        a.setflags(write=False)
    return bases, offs, keys, counts


# ---- 1. layouts ----------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,pool,canon", CONFIGS)
def test_layouts(mode, k, pool, canon):
    bases, offs, keys, counts = layout_case(k, canon)
    # the filter's scan spans many workgroups (k > 32: the reference's u64 keys
    # of a longer window collide, far fewer are distinct)
    assert keys.size > (64 if k <= 32 else 8) * 4096
    g = run(bases, offs, k, pool, canon, **mode)
    check_all(g, keys, counts)


# ---- 2. range filter -----------------------------------------------------------
@pytest.mark.parametrize("mode", [dict(exact=True), dict(exact=True, NK_EXACT_SORT=1)],
                         ids=["grouped", "sorted"])
def test_range_filter(mode):
    k, pool, canon = CONFIGS[0]
    bases, offs, keys, counts = layout_case(k, canon)
    g = run(bases, offs, k, pool, canon, **mode)
    assert counts.max() > 7 and (counts == 1).any()
    nothing = int(counts.max()) + 1
    for lo, hi in ((2, U32_MAX), (1, 1), (3, 7), (nothing, nothing + 5), (0, U32_MAX), (0, 0)):
        m = (counts >= max(lo, 1)) & (counts <= hi)
        gk, gc = g.counts_arrays(lo, hi)
        np.testing.assert_array_equal(gk, keys[m])
        np.testing.assert_array_equal(gc, counts[m])
        assert g.count_total(lo, hi) == int(m.sum())  # cap = 0 sizes the result
    for lo, hi in ((1, U32_MAX), (2, U32_MAX)):  # cap below the total: the first pairs
        m = (counts >= lo) & (counts <= hi)
        cap = 1234
        kb = np.full(cap + 1, 0xABCD, np.uint64)
        cb = np.full(cap + 1, 0xABCD, np.uint32)
        total = g._L.nk_export_counts(g._h, lo, hi, kb.ctypes.data, cb.ctypes.data, cap)
        assert total == int(m.sum()) > cap
        np.testing.assert_array_equal(kb[:cap], keys[m][:cap])
        np.testing.assert_array_equal(cb[:cap], counts[m][:cap])
        assert kb[cap] == 0xABCD and cb[cap] == 0xABCD  # nothing past cap
        gk, gc = g.counts_arrays(lo, hi, cap=cap)
        np.testing.assert_array_equal(gk, keys[m][:cap])
        np.testing.assert_array_equal(gc, counts[m][:cap])
    with pytest.raises(_lib.NeuroKmerError) as e:
        g.counts_arrays(5, 4)
    assert e.value.code == _lib.NK_E_INVALID
    with pytest.raises(_lib.NeuroKmerError):
        g.counts_device(5, 4)
    for nb in (1, 2**20 + 1):
        with pytest.raises(_lib.NeuroKmerError) as e:
            g.spectrum(nb)
        assert e.value.code == _lib.NK_E_INVALID
    for nb in (2, 3, 8192, 8193, 8194):  # around the LDS histogram's size
        np.testing.assert_array_equal(g.spectrum(nb), expected_spectrum(counts, nb))


# ---- 3. key 0 and holes ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def poly_a_case():
    rnd, _ = synth.make_records(300_000, 1, seed=5)
    bases = np.concatenate([np.full(400_000, ord("A"), np.uint8), rnd,
                            np.frombuffer(b"AAAAT" * 20_000, np.uint8)])
    offs = np.array([0, 400_000, 700_000, bases.size], np.uint64)
    keys, counts = expected(records(bases, offs), 31, True)
    return bases, offs, keys, counts


@pytest.mark.parametrize("exact", [True, False], ids=["fused", "standalone"])
def test_key_zero_and_holes(exact):
    bases, offs, keys, counts = poly_a_case()
    assert keys[0] == 0 and counts[0] > 399_000
    g = run(bases, offs, 31, 2_000_000, True, exact=exact)
    gk, gc = g.counts_arrays()
    assert int((gk == 0).sum()) == 1 and gk[0] == 0 and gc[0] == counts[0]
    check_all(g, keys, counts, bins=(100, 500_000))
    h = g.spectrum(500_000)  # a bin of its own, past the LDS range
    assert h[int(counts[0])] == int((counts == counts[0]).sum()) >= 1
    assert g.spectrum(100)[99] == int((counts >= 99).sum()) >= 1  # the high bin


# ---- 4. key ~0 -------------------------------------------------------------------
@pytest.mark.parametrize("mode", [dict(exact=True), dict(exact=True, NK_XHASH_MAX=8)],
                         ids=["grouped", "side"])
@pytest.mark.parametrize("run_t", [5_000, 90])
def test_all_t_key_k32(mode, run_t):
    rnd, _ = synth.make_records(50_000, 1, seed=9)
    bases = np.concatenate([rnd[:20_000], np.full(run_t, ord("T"), np.uint8), rnd[20_000:],
                            np.full(40, ord("t"), np.uint8)])
    offs = np.array([0, 30_000, bases.size], np.uint64)
    keys, counts = expected(records(bases, offs), 32, False)
    assert keys[-1] == 2**64 - 1
    g = run(bases, offs, 32, 3_001, False, **mode)
    gk, gc = g.counts_arrays()
    assert gk[-1] == 2**64 - 1 and gc[-1] == counts[-1]
    check_all(g, keys, counts)


# ---- 5. the process_sequence delta ----------------------------------------------
def delta_inputs():
    bases, offs = synth.make_records(120_000, 3, seed=12, repeats_per_mb=1000)
    seqs = (bases[1000:1400].tobytes(), b"ACGTTGCA" * 30, bases[50_000:50_100].tobytes())
    return bases, offs, seqs


def check_delta(g, recs):
    keys, counts = expected(recs, 15, True)
    kpn = g.kmer_per_neuron()
    check_all(g, keys, counts)
    gk, gc = g.counts_arrays()
    cnt, pres = g.get_counts(gk)
    assert pres.all()
    np.testing.assert_array_equal(cnt, gc)
    np.testing.assert_array_equal(g.kmer_per_neuron(), kpn)  # the export changes nothing
    m = counts >= 2
    gk, gc = g.counts_arrays(2)
    np.testing.assert_array_equal(gk, keys[m])
    np.testing.assert_array_equal(gc, counts[m])


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
    check_delta(g, recs)
    # a later process call replaces `counts`, delta included
    g.process_parallel_arrays(bases, offs)
    keys, counts = expected(records(bases, offs), 15, True)
    check_all(g, keys, counts)


def test_delta_without_a_table():
    _, _, seqs = delta_inputs()
    g = SpikingKmerCounter(15, 1.0, 0.95, 2, 1.0, 9_973, True, exact_counts=True)
    for seq in seqs:
        g.process_sequence(seq)
    check_delta(g, list(seqs))


def test_delta_all_t_key():
    """The delta keeps the key ~0 (its empty-slot marker) beside its slots."""
    g = SpikingKmerCounter(32, 1.0, 0.95, 2, 1.0, 3_001, False, exact_counts=True)
    seqs = [b"T" * 40 + b"ACGT" * 20, b"GATTACA" * 9 + b"T" * 33]
    for seq in seqs:
        g.process_sequence(seq)
    keys, counts = expected(seqs, 32, False)
    assert keys[-1] == 2**64 - 1 and counts[-1] == 11
    check_all(g, keys, counts)


# ---- 6. 128-bit keys ---------------------------------------------------------------
@pytest.mark.parametrize("k", [40, 64])
def test_kmer_width_128(k):
    bases, offs = synth.make_records(60_000, 3, repeats_per_mb=3000, motif_len=150, seed=k)
    cnt = collections.Counter()
    for rec in records(bases, offs):
        cnt.update(int(x) for x in cbind.kmer_keys128(rec, k, True))
    keys = sorted(cnt)
    counts = np.array([cnt[x] for x in keys], np.uint32)
    g = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, 50_021, True, kmer_width=128, exact_counts=True)
    g.process_parallel_arrays(bases, offs)
    gk, gc = g.counts_arrays()
    assert isinstance(gk, list) and gk == keys  # ascending as u128
    np.testing.assert_array_equal(gc, counts)
    assert any(x >> 64 for x in gk)
    for nb in (16, 5000):
        np.testing.assert_array_equal(g.spectrum(nb), expected_spectrum(counts, nb))
    assert counts.max() >= 2
    m = counts >= 2
    gk, gc = g.counts_arrays(2)
    assert gk == [x for x, keep in zip(keys, m) if keep]
    np.testing.assert_array_equal(gc, counts[m])
    gk, gc = g.counts_arrays(1, U32_MAX, cap=100)
    assert gk == keys[:100]
    np.testing.assert_array_equal(gc, counts[:100])


# ---- 7. replace and reset ------------------------------------------------------------
def test_replace_reset_and_unsupported():
    a, ao = synth.make_records(200_000, 3, seed=1, repeats_per_mb=500)
    b, bo = synth.make_records(150_000, 2, seed=2)
    for exact in (True, False):
        g = SpikingKmerCounter(25, 1.0, 0.95, 2, 1.0, 70_001, True, exact_counts=exact)
        assert g.counts_arrays()[0].size == 0 and not g.spectrum(50).any()  # fresh: empty
        g.process_parallel_arrays(a, ao)
        g.process_parallel_arrays(b, bo)
        check_all(g, *expected(records(b, bo), 25, True))
        g.reset()
        gk, gc = g.counts_arrays()
        assert gk.size == 0 and gc.size == 0 and g.count_total() == 0
        assert not g.spectrum(10001).any()
    d_b = torch.from_numpy(np.concatenate([b, np.zeros(16, np.uint8)])).cuda()
    d_o = torch.from_numpy(bo.view(np.int64)).cuda()
    torch.cuda.synchronize()
    g = SpikingKmerCounter(25, 1.0, 0.95, 2, 1.0, 70_001, True, exact_counts=False)
    g.process_parallel_device(d_b.data_ptr(), d_o.data_ptr(), 2, b.size)
    for call in (g.counts_arrays, g.counts_device, g.spectrum):
        with pytest.raises(_lib.NeuroKmerError) as e:
            call()
        assert e.value.code == _lib.NK_E_UNSUPPORTED
    g = SpikingKmerCounter(25, 1.0, 0.95, 2, 1.0, 70_001, True, exact_counts=True)
    g.process_parallel_device(d_b.data_ptr(), d_o.data_ptr(), 2, b.size)
    check_all(g, *expected(records(b, bo), 25, True))


# ---- 8. device variant, 9. determinism ---------------------------------------------
def from_device(ptr, n, dtype):
    out = np.zeros(max(n, 1), dtype)
    if n:
        _lib.copy_from_device(out.ctypes.data, ptr, n * out.itemsize)
    return out[:n]


@pytest.mark.parametrize("rng", [(1, U32_MAX), (2, 9)], ids=["all", "filtered"])
def test_device_variant_and_determinism(rng):
    k, pool, canon = CONFIGS[1]
    bases, offs, keys, counts = layout_case(k, canon)
    g = run(bases, offs, k, pool, canon)
    g2 = run(bases, offs, k, pool, canon)
    total = g.count_total(*rng)
    hk, hc = g.counts_arrays(*rng, cap=total)  # the host entry point
    s = torch.cuda.Stream()
    kp, cp, n = g.counts_device(*rng, stream=s.cuda_stream)  # complete on return
    assert n == total and kp and cp
    np.testing.assert_array_equal(from_device(kp, n, np.uint64), hk)
    np.testing.assert_array_equal(from_device(cp, n, np.uint32), hc)
    m = (counts >= rng[0]) & (counts <= rng[1])
    np.testing.assert_array_equal(hk, keys[m])
    k2, c2 = g2.counts_arrays(*rng)
    np.testing.assert_array_equal(k2, hk)
    np.testing.assert_array_equal(c2, hc)
    np.testing.assert_array_equal(g2.spectrum(), g.spectrum())


# ---- 10. CLI ---------------------------------------------------------------------
def test_cli_spectrum_and_counts(tmp_path):
    bases, offs = synth.make_records(50_000, 4, repeats_per_mb=4000, motif_len=80, seed=77)
    recs = records(bases, offs)
    fa = tmp_path / "in.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
    keys, counts = expected(recs, 21, True)
    base = [_lib.CLI_PATH, "-i", str(fa), "-k", "21", "--pool-size", "4001", "--canonical"]
    plain = subprocess.run(base, capture_output=True, check=True).stdout
    sp, ct = tmp_path / "spec.txt", tmp_path / "counts.tsv"
    out = subprocess.run(base + ["--spectrum", str(sp), "--counts", str(ct)],
                         capture_output=True, check=True).stdout
    assert out == plain
    lines = ct.read_text().splitlines()
    assert len(lines) == keys.size
    got_k = np.array([int(cbind.kmer_keys(ln.split("\t")[0].encode(), 21, True)[0]) for ln in lines],
                     np.uint64)
    assert all(len(ln.split("\t")[0]) == 21 for ln in lines)
    np.testing.assert_array_equal(got_k, keys)  # the right k-mers, in key order
    np.testing.assert_array_equal(np.array([int(ln.split("\t")[1]) for ln in lines]), counts)
    h = expected_spectrum(counts, 10002)
    assert sp.read_text().splitlines() == [f"{j} {int(h[j])}" for j in range(1, h.size) if h[j]]
    # --min-count and --spectrum-max
    out = subprocess.run(base + ["--spectrum", str(sp), "--spectrum-max", "3", "--counts", str(ct),
                                 "--min-count", "2"], capture_output=True, check=True).stdout
    assert out == plain
    assert len(ct.read_text().splitlines()) == int((counts >= 2).sum())
    h = expected_spectrum(counts, 5)
    assert sp.read_text().splitlines() == [f"{j} {int(h[j])}" for j in range(1, 5) if h[j]]
    # k > 32: the keys are not k-mers
    r = subprocess.run([_lib.CLI_PATH, "-i", str(fa), "-k", "40", "--pool-size", "4001",
                        "--counts", str(ct)], capture_output=True)
    assert r.returncode != 0 and b"--counts" in r.stderr
