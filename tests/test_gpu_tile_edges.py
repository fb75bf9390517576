"""The count kernels on records placed at tile, lane and chunk edges.

Every count kernel stages its input through stage_tile / window_key*
(neurokmer_amd/csrc/nk_tile.h).  oracle/tile_edges.py puts record ends, empty
and short records, invalid bytes, the end of the input and the first counted
position (accumulate_device_from) at fixed distances from the 4096- and
8192-position tile edges, the 16-position lanes, the 16-byte chunks and the
32-position words of the record-end mask; each count path (K1a, the generic
and wide partitions, the direct-atomic kernels, 64- and 128-bit keys, the
exact table) runs them.  Every comparison is bit-exact against
cbind.OracleCounter through test_gpu_parity.assert_same, whose top rows carry
the uniques of the rescans (k_uniq_scan / k_uniq_lanes / k_uniq_gen /
k_uniq_tiles) over the same edges.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")  # import first: one shared HIP runtime
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from neurokmer_amd import SpikingKmerCounter  # noqa: E402
from oracle import cbind  # noqa: E402
from oracle import tile_edges as TE  # noqa: E402
from test_gpu_parity import _keys_of, assert_exact_same, assert_same, run_both  # noqa: E402


@contextlib.contextmanager
def env(kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def layout(k, dirty, twins=True):
    bases, offs = TE.edge_layout(k, dirty=dirty, twins=twins)
    bases.setflags(write=False)  # shared among the cases
    return bases, offs


def upload(bases, offs):
    """Device copies as run_both makes them: 16 zero bytes after the bases."""
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros(16, np.uint8)])).cuda()
    d_o = torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return d_b, d_o


# ---- the path matrix ------------------------------------------------------------
@pytest.mark.parametrize("case", TE.path_cases(), ids=TE.case_id)
def test_edges_on_every_count_path(case):
    bases, offs = layout(case.k, case.dirty)
    with env(case.env):
        g, r = run_both(bases, offs, case.k, case.pool, case.canon, width=case.width)
    assert_same(g, r)
    assert int(g.currents().sum()) == TE.n_kmers(offs, case.k)
    g.close()


@pytest.mark.parametrize("case", TE.uniq_cases(), ids=TE.case_id)
def test_edges_through_the_uniques_rescans(case):
    """Every neuron a top row: each window of the layout is keyed again by the
    uniques rescan of its count path (k_uniq_scan, k_uniq_gen, k_uniq_lanes /
    k_uniq_tiles, the direct-atomic kernels' second mode), and every row's
    uniques column is compared.  With the twins a wrong key shows, without
    them a dropped window (oracle/tile_edges.py TWIN_SHIFT)."""
    bases, offs = layout(case.k, case.dirty, case.twins)
    with env(case.env):
        g, r = run_both(bases, offs, case.k, case.pool, case.canon, width=case.width,
                        top_n=case.pool)
    assert_same(g, r, n=case.pool)
    rows = g.top_abundant_neurons(case.pool)
    assert len(rows) == case.pool and sum(u for _, _, u in rows) == r.distinct_kmers()
    g.close()


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
def test_edges_streaming_lif_rule(dirty):
    bases, offs = layout(31, dirty)
    g, r = run_both(bases, offs, 31, 40_000, True, streaming=True, thr=0.0)
    assert_same(g, r)
    g.close()


# ---- the exact table ------------------------------------------------------------
@pytest.mark.parametrize("k,width,canon,pool", TE.EXACT_CASES)
def test_edges_exact_table(k, width, canon, pool):
    """K1a<KEYS>'s window_key on the sorted records and nk_exact.hip's
    4096-position tiles: kmer_per_neuron, distinct k-mers, get_count of every
    key of the input and of absent ones."""
    bases, offs = layout(k, not canon)
    g = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, canon, kmer_width=width, exact_counts=True)
    r = cbind.OracleCounter(k, 1.0, 0.95, 2, 1.0, pool, canon, width=width)
    g.process_parallel_arrays(bases, offs)
    r.process_parallel_arrays(bases, offs)
    assert_same(g, r)
    if width == 64:
        assert_exact_same(g, r, _keys_of(bases, offs, k, canon), pool)
    else:
        np.testing.assert_array_equal(g.kmer_per_neuron(), r.kmer_per_neuron())
        assert g.distinct_kmers() == r.distinct_kmers()
        keys = set()
        for i in range(offs.size - 1):
            keys.update(cbind.kmer_keys128(bases[int(offs[i]):int(offs[i + 1])].tobytes(), k, canon))
        rng = np.random.default_rng(k)
        probe = sorted(keys)
        probe += [int(a) | (int(b) << 64) for a, b in zip(rng.integers(0, 2**63, 300, dtype=np.uint64),
                                                           rng.integers(0, 2**20, 300, dtype=np.uint64))]
        cnt, pres = g.get_counts128(probe)
        for kk, c, p in zip(probe, cnt, pres):
            assert (int(c) if p else None) == r.get_count(kk), hex(kk)
    g.close()


# ---- the end of the input ---------------------------------------------------------
def _tid(cfg):
    k, width, e, canon, _ = cfg
    how = "-".join(x.split("_")[1].lower() for x in e) or "default"
    return f"k{k}-w{width}-{how}-{'canon' if canon else 'packed'}"


@pytest.mark.parametrize("cfg", TE.TAIL_CONFIGS, ids=_tid)
def test_input_ends_at_every_residue(cfg):
    """Inputs of T + r bases (oracle/tile_edges.py tail_inputs) on one handle,
    reset between them: the input ends on a tile edge, leaves a last tile with
    fewer than k bases, or ends in a partial 16-byte chunk; each with a twin
    of its last bases and without (oracle/tile_edges.py TWIN_SHIFT)."""
    k, width, e, canon, pool = cfg
    rows = min(pool, 1024)
    g = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, canon, kmer_width=width, top_n=rows)
    with env(e):
        for T, r_, bases, offs in TE.tail_inputs(k) + TE.tail_inputs(k, twins=False):
            r = cbind.OracleCounter(k, 1.0, 0.95, 2, 1.0, pool, canon, width=width)
            g.process_parallel_arrays(bases, offs)
            r.process_parallel_arrays(bases, offs)
            try:
                assert_same(g, r, n=rows)
            except AssertionError as err:
                raise AssertionError(f"n_bases = {T} + {r_}") from err
            g.reset()
    g.close()


@pytest.mark.parametrize("atomic", [False, True], ids=["default", "atomic"])
@pytest.mark.parametrize("canon", [True, False], ids=["canon", "packed"])
@pytest.mark.parametrize("k", [3, 21])
def test_more_records_in_a_tile_than_threads(k, canon, atomic):
    bases, offs = TE.many_records_tile()
    with env({"NK_FORCE_ATOMIC": "1"} if atomic else {}):
        g, r = run_both(bases, offs, k, 5003, canon)
    assert_same(g, r)
    assert int(g.currents().sum()) == TE.n_kmers(offs, k)
    g.close()


# ---- the first counted position (accumulate_device_from) --------------------------
@pytest.mark.parametrize("k,width,e,pool", TE.CUT_CONFIGS,
                         ids=["part", "gen-compat", "wide-rolled64", "gen-rolled128"])
def test_cuts_at_lane_offsets(k, width, e, pool):
    """Windows before first_pos counted on one handle from the input truncated
    to first_pos + k - 1 bases, the rest on another with
    accumulate_device_from(first_pos): together the whole input's currents,
    for first_pos at lane offsets 0, 1, 15, 16, 17 and -1 from a 16-aligned
    position inside a tile and from an edge of both tile sizes."""
    bases, offs = layout(k, False)
    r = cbind.OracleCounter(k, 1.0, 0.95, 2, 1.0, pool, True, width=width)
    r.process_parallel_arrays(bases, offs)
    want = r.currents()
    a = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, True, kmer_width=width)
    b = SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, True, kmer_width=width)
    d_b, d_o = upload(bases, offs)
    for q in TE.cut_bases(k):
        for j in TE.CUT_J:
            p = q + j
            tb, to = TE.truncate(bases, offs, p + k - 1)
            d_tb, d_to = upload(tb, to)
            with env(e):
                a.accumulate_device(d_tb.data_ptr(), d_to.data_ptr(), to.size - 1, tb.size)
                b.accumulate_device_from(d_b.data_ptr(), d_o.data_ptr(), offs.size - 1, bases.size, p)
            ca, cb = a.currents(), b.currents()
            assert int(ca.sum()) == TE.n_kmers(to, k), (q, j)
            assert int(ca.sum()) + int(cb.sum()) == int(want.sum()), (q, j)
            np.testing.assert_array_equal(ca + cb, want, err_msg=f"first_pos = {q} + {j}")
    a.close()
    b.close()
