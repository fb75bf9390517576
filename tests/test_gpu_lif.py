"""The LIF and top-N kernels on injected currents, against the step-by-step loop.

Count vectors are written straight into the currents buffer (what an
all-reduce leaves there) and nk_finalize runs the LIF and the selection on
them, so the closed form (nk_device.h lif_closed), its table of fresh neurons,
the derived state, the carried state and the selection passes see counts,
parameters and spike vectors that k-mer counts of synthetic DNA never give
them (oracle/lif_grid.py).  The reference is `steps` calls of
LifNeuron::update per neuron (oracle/nk_oracle.c nko_lif); everything is
bit-exact.  No input is counted, so every row's uniques column is 0.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")  # import first: one shared HIP runtime
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from neurokmer_amd import SpikingKmerCounter, synth  # noqa: E402
from oracle import cbind  # noqa: E402
from oracle import lif_grid as G  # noqa: E402

POOL = 8193  # one full LIF block (8192 neurons) plus one; not a multiple of 8


class _CAI:
    def __init__(self, ptr, n, typestr="<i8"):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False),
                                         "version": 3}


def inject(g, counts):
    """counts (u64) -> the handle's currents buffer."""
    counts = np.ascontiguousarray(counts, np.uint64)
    t = torch.from_numpy(counts.view(np.int64)).cuda()
    cur = torch.as_tensor(_CAI(g.device_currents_ptr(), counts.size), device="cuda")
    cur.copy_(t)
    torch.cuda.synchronize()


def counter(thr=1.0, leak=0.95, refr=2, steps=1000, pool=POOL, cost=1.0, top_n=20):
    g = SpikingKmerCounter(31, thr, leak, refr, cost, pool, True, top_n=top_n)
    g.set_steps(steps)
    return g


def assert_state(g, R, cost=1.0, n=20):
    np.testing.assert_array_equal(g.voltages().view(np.uint32), R.v)
    np.testing.assert_array_equal(g.refractory(), R.r)
    np.testing.assert_array_equal(g.spike_counts(), R.spikes)
    total = int(R.spikes.sum())
    assert g.energy.total_spikes() == total
    assert g.energy_used() == G.energy(total, cost)
    assert g.top_abundant_neurons(n) == G.top_rows(R.spikes, n)


def _pid(p):
    return "thr%s-leak%s-refr%s" % p


# ---- 3a: the grid -------------------------------------------------------------
@pytest.mark.parametrize("streaming", [False, True], ids=["inmem", "streaming"])
@pytest.mark.parametrize("params", G.PARAMS, ids=_pid)
def test_grid(params, streaming):
    """Round 1: fresh neurons, the derived state (table rows, and the closed
    form past row 65535); rounds 2 and 3: the carried state."""
    thr, leak, refr = params
    rs = G.rounds(POOL)
    for steps in G.STEPS:
        ex = G.expected(rs, steps, thr, leak, refr, streaming)
        g = counter(thr, leak, refr, steps)
        for cnts, R in zip(rs, ex):
            inject(g, cnts)
            g.finalize(streaming)
            assert_state(g, R)
        g.close()


@pytest.mark.parametrize("streaming", [False, True], ids=["inmem", "streaming"])
def test_table_edge_at_rest_on_a_used_handle(streaming):
    """A neuron at rest (v == 0, r == 0) on a handle that is no longer fresh
    takes its table row when its count is below 65536 and the closed form from
    there on.  No spike at this threshold, so v ends at the sum of the currents
    and tells row 65535 from count 65536; round 3 meets the same counts with a
    carried voltage."""
    thr, leak, refr = 16777216.0, 1.0, 0
    edge = np.array([0, 65534, 65535, 65536, 65537, 1, 65535, 65536, 131071], np.uint64)
    edge = edge[np.arange(POOL) % edge.size]
    rs = [np.zeros(POOL, np.uint64), edge, edge]
    for steps in (1, 3, 1000):
        ex = G.expected(rs, steps, thr, leak, refr, streaming)
        assert not ex[0].v.any() and not ex[0].r.any()  # at rest after round 1
        assert len(set(ex[1].v[2:5].tolist())) == 3     # 65535, 65536, 65537 end apart
        g = counter(thr, leak, refr, steps)
        for cnts, R in zip(rs, ex):
            inject(g, cnts)
            g.finalize(streaming)
            assert_state(g, R)
        g.close()


# ---- 3b: read order of the derived state --------------------------------------
@pytest.mark.parametrize("top_n", [20, 100])  # selected inside the LIF kernel / by the select kernels
@pytest.mark.parametrize("rows_first", [True, False])
def test_derived_state_read_order(rows_first, top_n):
    """After the first finalize v / r / spike counts are a function of the
    counts and not written out.  Rows past top_n read first: the selection
    derives the spikes from the counts.  A state array read first: the state
    is settled, and the selection reads the written spike counts."""
    cnts = G.rounds(POOL)[0]
    R = G.expected([cnts], 1000, 1.0, 0.95, 2, False)[0]
    g = counter(top_n=top_n)
    inject(g, cnts)
    g.finalize(False)
    assert g.top_abundant_neurons(top_n) == G.top_rows(R.spikes, top_n)
    if rows_first:
        assert g.top_abundant_neurons(500) == G.top_rows(R.spikes, 500)
        np.testing.assert_array_equal(g.spike_counts(), R.spikes)
    else:
        np.testing.assert_array_equal(g.spike_counts(), R.spikes)
        assert g.top_abundant_neurons(500) == G.top_rows(R.spikes, 500)
    assert g.top_abundant_neurons(POOL) == G.top_rows(R.spikes, POOL)
    assert_state(g, R)
    g.close()


# ---- 3c: simulate_spikes_auto ------------------------------------------------
@pytest.mark.parametrize("thr", [1.0, 0.0])  # 0.0: a zero count fires under this rule
def test_simulate_spikes_auto_on_injected_currents(thr):
    """The streaming rule over the held currents (zero counts stepped too),
    twice, then steps 0 (nothing happens), then another steps value.  That the
    oracle's simulate_spikes_auto is this loop: tests/test_lif_grid.py."""
    cnts = G.rounds(POOL)[0]
    ex = G.expected([cnts] * 3, [1000, 1000, 333], thr, 0.95, 2, True)
    g = counter(thr=thr)
    inject(g, cnts)
    g.simulate_spikes_auto()
    assert_state(g, ex[0])
    g.simulate_spikes_auto()
    assert_state(g, ex[1])
    g.set_steps(0)
    g.simulate_spikes_auto()
    assert_state(g, ex[1])
    g.set_steps(333)
    g.simulate_spikes_auto()
    assert_state(g, ex[2])
    np.testing.assert_array_equal(g.currents(), cnts)
    g.close()


# ---- 3d: steps 0 ---------------------------------------------------------------
@pytest.mark.parametrize("streaming", [False, True], ids=["inmem", "streaming"])
def test_steps_zero_changes_nothing(streaming):
    cnts = G.rounds(POOL)[0]
    g = counter(steps=0)
    inject(g, cnts)
    g.finalize(streaming)
    assert not g.voltages().view(np.uint32).any()
    assert not g.refractory().any() and not g.spike_counts().any()
    assert g.energy.total_spikes() == 0 and g.energy_used() == 0.0
    assert g.top_abundant_neurons(20) == [(i, 0, 0) for i in range(20)]
    # and from a carried state: a round at 1000 steps, then steps 0
    R = G.expected([cnts], 1000, 1.0, 0.95, 2, streaming)[0]
    g.set_steps(1000)
    g.finalize(streaming)
    g.set_steps(0)
    g.finalize(streaming)
    assert_state(g, R)
    g.finalize(streaming)
    assert_state(g, R)
    g.close()


# ---- 3e: set_steps / the other rule between a count and its finalize ----------
@pytest.mark.parametrize("case", ["steps", "streaming-thr0"])
def test_count_then_other_lif_settings(case):
    """accumulate_device may already have run the in-memory LIF at the steps it
    saw (the write-through histogram: compat keys, one workgroup per bucket, a
    selection not fused into the LIF kernel); a finalize at other steps, or
    with the streaming rule at a threshold a zero count reaches, must not use
    it (nk_finish.cpp k1b_lif_holds)."""
    k, pool, top_n = 33, 4_300_003, 100
    thr = 0.0 if case == "streaming-thr0" else 1.0
    bases, offs = synth.make_records(50_000, 3, seed=77, repeats_per_mb=20_000, motif_len=60)
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros(16, np.uint8)])).cuda()
    d_o = torch.from_numpy(offs.view(np.int64)).cuda()
    torch.cuda.synchronize()
    g = SpikingKmerCounter(k, thr, 0.95, 2, 1.0, pool, True, top_n=top_n)
    r = cbind.OracleCounter(k, thr, 0.95, 2, 1.0, pool, True)
    assert g.get_steps() == 1000
    g.accumulate_device(d_b.data_ptr(), d_o.data_ptr(), offs.size - 1, int(offs[-1]))
    if case == "steps":
        g.set_steps(700)
        r.set_steps(700)
        g.finalize(False)
        r.process_parallel_arrays(bases, offs)
    else:
        g.finalize(True)
        r.process_streaming_arrays(bases, offs)
    np.testing.assert_array_equal(g.currents(), r.currents())
    np.testing.assert_array_equal(g.spike_counts(), r.spike_counts())
    np.testing.assert_array_equal(g.voltages().view(np.uint32), r.voltages().view(np.uint32))
    np.testing.assert_array_equal(g.refractory(), r.refractory())
    assert g.energy.total_spikes() == r.total_spikes
    assert g.energy_used() == r.energy_used()
    assert g.top_abundant_neurons(top_n) == r.top_abundant_neurons(top_n)
    g.close()


# ---- 4: the selection at chosen spike vectors ----------------------------------
# thr 1, leak 0, no refractory period: a neuron whose count equals `steps` fires
# on every step of the round, one with count 0 never.  Rounds at steps 1, 2, 4,
# ... 4096 give neuron i exactly target[i] spikes, any value in 0..8191.
BITS = 13
TOP_NS = (1, 63, 64, 65, 333)  # <= 64 rows: selected inside the LIF kernel


def drive(target, top_n):
    """A counter taken through the 13 rounds; the rows of every round are
    checked on the way (each prefix of the bits is a spike vector too)."""
    target = np.asarray(target, np.uint64)
    assert int(target.max()) < 1 << BITS
    steps = [1 << b for b in range(BITS)]
    rs = [np.where((target >> np.uint64(b)) & np.uint64(1), np.uint64(1 << b), np.uint64(0))
          for b in range(BITS)]
    ex = G.expected(rs, steps, 1.0, 0.0, 0, False)
    np.testing.assert_array_equal(ex[-1].spikes, target)
    g = counter(1.0, 0.0, 0, 1, pool=target.size, top_n=top_n)
    for cnts, st, R in zip(rs, steps, ex):
        g.set_steps(st)
        inject(g, cnts)
        g.finalize(False)
        assert g.top_abundant_neurons(top_n) == G.top_rows(R.spikes, top_n), st
    return g


def check_selection(target, top_n):
    target = np.asarray(target, np.uint64)
    pool = target.size
    g = drive(target, top_n)
    # rows past top_n: the select kernels up to 1024 rows, the ranked pool past that
    for n in (top_n, top_n + 7, 1024, 1025, pool):
        assert g.top_abundant_neurons(n) == G.top_rows(target, n), n
    np.testing.assert_array_equal(g.spike_counts(), target)
    assert g.energy.total_spikes() == int(target.sum())
    for n in (top_n, top_n + 7, pool):  # again, from the settled state
        assert g.top_abundant_neurons(n) == G.top_rows(target, n), n
    g.close()


def cut_vector(pool, top_n, tie, hi, seed):
    """A spike vector whose top_n-th row falls inside a run of 2000 neurons
    tied at `tie` (so do the 1024th and 1025th): top_n // 2 neurons above it,
    spread over tie + 1 .. hi with `hi` itself among them, everything else
    below it down to 0; ties and winners on both sides of the LIF block
    boundary, the pool's last neuron a tie."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, tie, pool).astype(np.uint64)  # below the run
    t[rng.random(pool) < 0.3] = 0
    t[rng.random(pool) < 0.1] = tie - 1
    idx = rng.permutation(pool - 1)
    n_above = top_n // 2
    above = rng.integers(tie + 1, hi + 1, n_above).astype(np.uint64)
    if n_above:
        above[0] = hi
    if n_above > 2:
        above[1] = above[2] = tie + 1  # ties above the cut too
    t[idx[:n_above]] = above
    t[idx[n_above:n_above + 1999]] = tie
    t[pool - 1] = tie
    assert (t > tie).sum() == n_above and (t == tie).sum() == 2000
    return t


@pytest.mark.parametrize("top_n", TOP_NS)
def test_selection_sparse_and_uniform(top_n):
    rng = np.random.default_rng(top_n)
    # every neuron the same count: past the one-byte copy and in the last bin
    check_selection(np.full(POOL, 4095, np.uint64), top_n)
    # fewer than top_n spiking neurons: the rest are zero-spike rows in index order
    t = np.zeros(POOL, np.uint64)
    t[rng.permutation(POOL)[:top_n // 2]] = rng.integers(1, 600, top_n // 2).astype(np.uint64)
    check_selection(t, top_n)
    # exactly top_n
    t = np.zeros(POOL, np.uint64)
    t[rng.permutation(POOL - 1)[:top_n - 1]] = rng.integers(1, 600, top_n - 1).astype(np.uint64)
    t[POOL - 1] = 255
    assert np.count_nonzero(t) == top_n
    check_selection(t, top_n)


@pytest.mark.parametrize("top_n", TOP_NS)
def test_selection_cut_at_the_byte_limit(top_n):
    """The one-byte copy of the spike counts says "255 or more" at 255."""
    for tie in (254, 255, 256):
        check_selection(cut_vector(POOL, top_n, tie, 300, 1000 * top_n + tie), top_n)


@pytest.mark.parametrize("top_n", TOP_NS)
def test_selection_cut_at_the_histogram_limit(top_n):
    """The last bin of the spike histogram says "4095 or more": the exact
    threshold comes from the radix refine on the host."""
    for tie in (4094, 4095, 4096):
        check_selection(cut_vector(POOL, top_n, tie, 8191, 1000 * top_n + tie), top_n)


@pytest.mark.parametrize("top_n", TOP_NS)
@pytest.mark.parametrize("pool", [8191, 8192, 8193, 16385])
def test_selection_winners_at_the_end_of_the_pool(pool, top_n):
    t = np.full(pool, 7, np.uint64)
    t[::3] = 0
    n = top_n + 3  # the last rows tie: the cut takes the lower indices
    t[pool - n:] = 300 + (np.arange(n) % 5).astype(np.uint64)
    g = drive(t, top_n)
    for m in (top_n, top_n + 7, pool):
        assert g.top_abundant_neurons(m) == G.top_rows(t, m), m
    np.testing.assert_array_equal(g.spike_counts(), t)
    g.close()


def test_selection_top_n_larger_than_the_pool():
    t = np.array([3, 0, 3, 8191, 0, 1, 255], np.uint64)
    g = drive(t, 20)
    assert g.top_abundant_neurons(20) == G.top_rows(t, 20)
    assert len(g.top_abundant_neurons(20)) == 7
    assert g.top_abundant_neurons(3) == G.top_rows(t, 3)
    np.testing.assert_array_equal(g.spike_counts(), t)
    g.close()


# ---- 5: the energy fixed point ---------------------------------------------------
@pytest.mark.parametrize("cost", [0.0, -1.0, G.NAN, 0.0004, 0.001, 0.0015, 2.5, 1.8e16, 1e17])
def test_energy_fixed_point(cost):
    """cost_fixed is Rust's `(cost * 1000.0) as u64`; the sum wraps modulo 2^64
    (at 1.8e16 the product does, at 1e17 the cost saturates first)."""
    cnts = np.zeros(100, np.uint64)
    cnts[[0, 5, 17, 40, 41, 98, 99]] = 4
    g = counter(1.0, 0.0, 0, 4, pool=100, cost=cost)
    inject(g, cnts)
    g.finalize(False)
    assert g.energy.total_spikes() == 28
    assert g.energy_used() == G.energy(28, cost) == g.energy.total_energy()
    inject(g, cnts)
    g.finalize(False)  # accumulates, wrapping again
    assert g.energy.total_spikes() == 56
    assert g.energy_used() == G.energy(56, cost)
    g.close()
