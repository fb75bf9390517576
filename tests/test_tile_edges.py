"""CPU tests of the placed-record layouts (oracle/tile_edges.py): the edges they
promise are there, no case is lost, and the reference side is pinned on
exactly these layouts (the C oracle against the pure-Python restatement)."""
import numpy as np
import pytest

from neurokmer_amd import synth
from oracle import cbind, pyref
from oracle import tile_edges as TE


def _ends_at(offs, E):
    """Distances of every record boundary within 70 bases of E."""
    o = offs.astype(np.int64)
    near = o[np.abs(o - E) <= 70] - E
    return set(int(x) for x in near)


@pytest.mark.parametrize("k", TE.all_ks())
def test_every_delta_at_both_tile_sizes(k):
    assert TE.all_ks() == [1, 5, 15, 16, 17, 21, 31, 32, 33, 40, 63, 64, 65]
    D = TE.deltas(k)
    assert set(D) >= {-64, -k - 1, -k, -k + 1, -17, -16, -15, -1, 0, 1, 15, 16, 17, 31, 32, 33,
                      k - 2, k - 1, k, 63, 64, 65}
    for dirty, twins in ((False, True), (True, True), (True, False)):
        bases, offs = TE.edge_layout(k, dirty=dirty, twins=twins)
        assert np.array_equal(offs, TE.edge_layout(k)[1])
        n = bases.size
        assert n == int(offs[-1]) and n % 16 == 5
        assert (np.diff(offs.astype(np.int64)) >= 0).all() and offs[0] == 0
        # every multiple of 4096 inside the input is an edge of the plan
        plan = TE.edge_plan(k)
        assert [E for E, _, _ in plan] == list(range(TE.TILE, n, TE.TILE))
        for tile in (TE.TILE, TE.PART_TILE):
            for d in D:
                # odd multiples of 4096 are no edge of the 8192-position tiles
                only = [E for E, what, _ in plan if what == d and
                        (E % TE.PART_TILE == 0 if tile == TE.PART_TILE else E % TE.PART_TILE != 0)]
                assert len(only) == 1, (tile, d)
                assert _ends_at(offs, only[0]) == {d}, (tile, d)


@pytest.mark.parametrize("k", TE.all_ks())
def test_extras_exist(k):
    bases, offs = TE.edge_layout(k)
    o = offs.astype(np.int64)
    starts, lens = o[:-1], np.diff(o)
    seen = {x: 0 for x in TE.EXTRAS}
    for E, what, _ in TE.edge_plan(k):
        if what == "empties":
            i = int(np.searchsorted(o, E, side="left"))
            assert o[i:i + 4].tolist() == [E] * 4 and o[i + 4] > E      # three empty records
        elif what == "straddle":
            m = (starts == E - (k - 1) // 2) & (lens == k - 1)
            assert m.sum() >= 1
            if k > 2:  # the record has a base on either side of the edge
                assert E - (k - 1) // 2 < E < E - (k - 1) // 2 + k - 1
        elif what == "single_before":
            assert ((starts == E - 1) & (lens == k)).sum() == 1
        elif what == "single_at":
            assert ((starts == E) & (lens == k)).sum() == 1
        else:
            continue
        seen[what] += 1
    assert seen == {x: 2 for x in TE.EXTRAS}  # one edge of each parity
    # everything else is a filler record of 200 .. 3000 bases
    filler = (lens >= 200) & (lens <= 3000)
    assert filler.sum() > 2 * len(TE.deltas(k)) and set(lens[~filler].tolist()) <= {0, k - 1, k}


def test_dirty_bytes():
    for k in (1, 31, 64):
        clean, offs = TE.edge_layout(k)
        dirty, offs2 = TE.edge_layout(k, dirty=True)
        assert np.array_equal(offs, offs2)
        assert set(np.unique(clean).tolist()) == set(b"ACGT")
        npos = TE.n_positions(k)
        assert (dirty[npos] == ord("N")).all()
        plan = TE.edge_plan(k)
        assert TE.n_offsets(k) == (-1, 0, k - 1, k, 47, 48, 63)
        assert {p - E for p, (E, _, _) in zip(npos, plan)} == set(TE.n_offsets(k))
        low = np.isin(dirty, np.frombuffer(b"acgt", np.uint8)).mean()
        assert 0.005 < low < 0.02
        assert np.isin(dirty, np.frombuffer(b"RYKMSWBDHV.-", np.uint8)).sum() >= 10
        same = dirty == clean
        assert same.mean() > 0.97


@pytest.mark.parametrize("dirty", [False, True])
def test_twins(dirty):
    """Every window near an edge, and the input's last windows, occur a second
    time inside one record: their keys matter to the uniques."""
    for k in (1, 31, 65):
        bases, offs = TE.edge_layout(k, dirty=dirty)
        o = offs.astype(np.int64)
        plan = TE.edge_plan(k)
        H, S = TE.TWIN_HALF, TE.TWIN_SHIFT
        assert H >= 65 + 65  # every window that touches a boundary placed at the edge
        for E, _, _ in plan:
            assert np.array_equal(bases[E - H:E + H], bases[E - H + S:E + H + S])
            r = int(np.searchsorted(o, E - H + S, side="right")) - 1
            assert o[r] <= E - H + S and E + H + S <= o[r + 1]
            assert o[r + 1] - o[r] == TE.TWIN_REC[1] - TE.TWIN_REC[0]
        last, n = plan[-1][0], bases.size
        at = last + TE.END_TWIN
        assert np.array_equal(bases[n - TE.END_LEN:], bases[at:at + TE.END_LEN])
        r = int(np.searchsorted(o, at, side="right")) - 1
        assert at + TE.END_LEN <= o[r + 1] and TE.END_LEN >= 65 + 16
    for k in (1, 31, 64):
        for T, r, b, _ in TE.tail_inputs(k):
            if T:
                assert np.array_equal(b[1000:1096], b[b.size - 96:])
            else:
                assert np.array_equal(b[3:], b[:-3])
        plain = TE.tail_inputs(k, twins=False)
        assert [(T, r, b.size) for T, r, b, _ in plain] == \
            [(T, r, b.size) for T, r, b, _ in TE.tail_inputs(k)]
        assert all(not np.array_equal(b[1000:1096], b[b.size - 96:]) for T, _, b, _ in plain if T)


def test_truncate():
    bases, offs = TE.edge_layout(31)
    b, o = TE.truncate(bases, offs, 5000)
    assert b.size == 5000 and o[0] == 0 and o[-1] == 5000 and o[-2] < 5000
    assert np.array_equal(o[:-1], offs[:o.size - 1])
    cut = int(offs[7])  # a cut on a record boundary keeps no empty record behind it
    b, o = TE.truncate(bases, offs, cut)
    assert o.tolist() == offs[:8].tolist()
    b, o = TE.truncate(bases, offs, bases.size)
    assert np.array_equal(o, offs)


def test_tail_inputs():
    counts = {1: 31, 16: 27, 31: 35, 32: 31, 33: 35, 63: 39, 64: 39}
    assert sorted({c[0] for c in TE.TAIL_CONFIGS}) == sorted(counts)
    for k, want in counts.items():
        cases = TE.tail_inputs(k)
        assert len(cases) == want
        assert len({(T, r) for T, r, _, _ in cases}) == want
        sizes = [b.size for _, _, b, _ in cases]
        assert all(s == T + r and s > 0 for s, (T, r, _, _) in zip(sizes, cases))
        assert {0, 1, 15} <= {s % 16 for s in sizes}
        assert any(T > 0 and r == 0 for T, r, _, _ in cases)          # ends on a tile edge
        if k > 1:
            assert any(T > 0 and 0 < r < k for T, r, _, _ in cases)   # a last tile without k-mers
        assert any(T > 0 and r == k for T, r, _, _ in cases)          # ... with exactly one
        for _, _, b, o in cases:
            assert o.size == 3 and o[0] == 0 and o[-1] == b.size and o[1] <= 3


def test_many_records_tile():
    bases, offs = TE.many_records_tile()
    lens = np.diff(offs.astype(np.int64))
    assert lens.size == 9001 and lens[-1] == 5000
    assert lens[:-1].min() == 1 and lens[:-1].max() == 3
    assert (offs < TE.TILE).sum() > 512 and (offs < TE.PART_TILE).sum() > 512
    assert TE.n_kmers(offs, 3) > 2000 and TE.n_kmers(offs, 21) == 4980


def test_case_counts():
    cases = TE.path_cases()
    assert len(cases) == 74
    assert len({TE.case_id(c) for c in cases}) == 74
    by_path = {}
    for c in cases:
        by_path.setdefault(c.path, set()).add(c.k)
    assert by_path == {"part-1": {1, 15, 16, 17, 31, 32}, "part-many": {16, 31, 32},
                       "part-xcd": {31}, "part-xcd-k1a": {31}, "gen-compat": {33, 63},
                       "gen-128": {33, 63, 64}, "wide": {31, 40}, "wide-128": {63},
                       "atomic": {16, 31, 40, 65}, "atomic-128": {17, 64}}
    assert all(c.dirty for c in cases if not c.canon)
    uniq = TE.uniq_cases()
    assert len(uniq) == len({TE.case_id(c) for c in uniq}) == 52
    assert all(c.pool <= 1024 for c in uniq)  # every neuron among the rows a handle selects
    assert len(TE.EXACT_CASES) == 4 and len(TE.TAIL_CONFIGS) == 22
    assert len(TE.CUT_CONFIGS) * 2 * len(TE.CUT_J) == 48


@pytest.mark.parametrize("k", sorted({c[0] for c in TE.CUT_CONFIGS}))
def test_cut_positions(k):
    bases, offs = TE.edge_layout(k)
    o = offs.astype(np.int64)
    mid, edge = TE.cut_bases(k)
    assert mid % 16 == 0 and mid % TE.TILE not in (0, TE.TILE - 16)
    assert edge % TE.PART_TILE == 0
    for q in (mid, edge):
        for j in TE.CUT_J:
            p = q + j
            r = int(np.searchsorted(o, p, side="right")) - 1
            assert p - o[r] >= 32 and o[r + 1] - p >= k


@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("k", [5, 31, 33])
def test_oracle_agrees_with_python_restatement(k, canon):
    """cbind.OracleCounter against oracle/pyref.py on the layout's first five
    edges (the dirty layout for the non-canonical keys)."""
    bases, offs = TE.edge_layout(k, dirty=not canon)
    bases, offs = TE.truncate(bases, offs, 5 * TE.TILE + 100)
    pool = 4099
    r = cbind.OracleCounter(k, 1.0, 0.95, 2, 1.0, pool, canon)
    r.process_parallel_arrays(bases, offs)
    p = pyref.SpikingKmerCounter(k, 1.0, 0.95, 2, 1.0, pool, canon)
    p.process_parallel(synth.records_list(bases, offs))
    assert r.currents().tolist() == p.currents
    assert r.spike_counts().tolist() == p.sc
    assert r.top_abundant_neurons(20) == p.top_abundant_neurons(20)
    assert int(r.currents().sum()) == TE.n_kmers(offs, k)


@pytest.mark.parametrize("k,width", [(k, w) for k in TE.all_ks() for w in (64, 128)
                                     if w == 64 or k <= 64])
def test_oracle_counts_every_window(k, width):
    for canon, dirty in ((True, False), (True, True), (False, True)):
        bases, offs = TE.edge_layout(k, dirty=dirty)
        r = cbind.OracleCounter(k, 1.0, 0.95, 2, 1.0, 5003, canon, width=width)
        r.process_parallel_arrays(bases, offs)
        assert int(r.currents().sum()) == TE.n_kmers(offs, k)
