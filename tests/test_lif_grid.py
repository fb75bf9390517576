"""CPU tests of the injected-current grid (oracle/lif_grid.py): it reaches every
branch class of the closed-form LIF, and the step-by-step checker it is built
on is LifNeuron::update (src/models.rs:34-51)."""
import collections

import numpy as np
import pytest

from neurokmer_amd import synth
from oracle import cbind
from oracle import lif_grid as G


@pytest.fixture(scope="module")
def grid():
    """Every (neuron, round) of PARAMS x STEPS x both rules over one period of
    COUNTS: [(params, steps, streaming, count, v_in, r_in, v, r, new, class)]."""
    rows = []
    rs = G.rounds(len(G.COUNTS))
    for thr, leak, refr in G.PARAMS:
        for steps in G.STEPS:
            for streaming in (False, True):
                for cnts, R in zip(rs, G.expected(rs, steps, thr, leak, refr, streaming)):
                    for i, c in enumerate(cnts):
                        a = (int(c), steps, thr, leak, refr, streaming, int(R.v_in[i]),
                             int(R.r_in[i]), int(R.v[i]), int(R.r[i]), int(R.new[i]))
                        rows.append(a + (G.outcome(*a),))
    return rows


def test_grid_reaches_every_class(grid):
    assert len(grid) == len(G.PARAMS) * len(G.STEPS) * 2 * len(G.COUNTS) * len(G.SHIFTS) == 19530
    seen = collections.Counter(row[-1] for row in grid)
    # a fresh neuron has no refractory ticks to drain, and a count past the
    # table is never the zero the in-memory rule skips
    want = [("fresh", "table", k) for k in ("skipped",) + G.SPIKING]
    want += [("carried", "table", k) for k in G.KINDS]
    want += [("fresh", "past", k) for k in G.SPIKING]
    want += [("carried", "past", k) for k in ("drain",) + G.SPIKING]
    missing = [w for w in want if not seen[w]]
    assert not missing, (missing, dict(seen))


def test_grid_fires_once_from_carried_voltage_only(grid):
    """One spike from the carried voltage although a fresh neuron with that
    count never fires (lif_closed: the second search from 0 does not reach the
    threshold).  Needs leak >= 1: with 0 <= leak < 1 the voltage from 0 bounds
    every later one.  `after`: steps were left to integrate after that spike's
    refractory period, so the neuron ends at the voltage of that search."""
    hits, after = 0, 0
    for count, steps, thr, leak, refr, streaming, v_in, r_in, v, r, new, cls in grid:
        if cls[0] != "carried" or cls[2] in ("skipped", "drain") or new != 1:
            continue
        if cbind.lif(count, steps, thr, leak, refr, not streaming)[2] != 0:
            continue
        assert leak >= 1.0
        hits += 1
        after += r == 0 and G.bits_f32(v) != 0.0
    assert hits >= 10 and after >= 1, (hits, after)


def _update(v, r, thr, leak, refr, c):
    """LifNeuron::update in numpy.float32: the product and the sum rounded
    separately, `>=` against the threshold."""
    if r > 0:
        return v, r - 1, 0
    v = np.float32(np.float32(v * leak) + c)
    if v >= thr:
        return np.float32(0.0), refr, 1
    return v, r, 0


@pytest.mark.parametrize("streaming", [False, True])
def test_checker_is_the_reference_update(streaming):
    thr, leak, refr = G.PARAMS[14]  # (1.0, 0.999, 7): long climbs, a real refractory period
    f_thr, f_leak = np.float32(thr), np.float32(leak)
    rs = G.rounds(len(G.COUNTS))
    for steps in (1, 7, 1003):
        ex = G.expected(rs, steps, thr, leak, refr, streaming)
        v = [np.float32(0.0)] * len(G.COUNTS)
        r = [0] * len(G.COUNTS)
        sc = [0] * len(G.COUNTS)
        with np.errstate(all="ignore"):
            for cnts, R in zip(rs, ex):
                for i, count in enumerate(int(x) for x in cnts):
                    if count or streaming:
                        c = G.current(count, steps)
                        for _ in range(steps):
                            v[i], r[i], s = _update(v[i], r[i], f_thr, f_leak, refr, c)
                            sc[i] += s
                assert [G.f32_bits(x) for x in v] == R.v.tolist()
                assert r == R.r.tolist()
                assert sc == R.spikes.tolist()


def test_expected_top_rows_and_energy():
    sp = np.array([3, 0, 7, 7, 2**40, 3, 0], np.uint64)
    assert G.top_rows(sp, 4) == [(4, 2**40, 0), (2, 7, 0), (3, 7, 0), (0, 3, 0)]
    assert len(G.top_rows(sp, 20)) == 7
    assert [G.cost_fixed(x) for x in (0.0, -1.0, G.NAN, 0.0004, 0.001, 0.0015, 2.5)] == \
        [0, 0, 0, 0, 1, 1, 2500]
    assert G.cost_fixed(1.8e16) == 18 * 10**18 and G.cost_fixed(1e17) == 2**64 - 1
    assert G.energy(3, 1.8e16) == float((54 * 10**18) % 2**64) / 1000.0
    assert G.energy(3, 1e17) == float(2**64 - 3) / 1000.0


def test_simulate_spikes_auto_is_the_streaming_loop():
    """OracleCounter.simulate_spikes_auto == cbind.lif per neuron with the
    streaming rule (zero counts stepped too), state carried, at thr = 0 where
    the two rules differ."""
    bases, offs = synth.make_records(3000, 2, seed=5)
    r = cbind.OracleCounter(9, 0.0, 0.95, 2, 1.0, 4099, True)
    r.set_steps(50)
    r.process_parallel_arrays(bases, offs)
    cur = r.currents()
    assert (cur == 0).any() and (cur > 0).any()
    # the in-memory call, then the streaming rule from that state, restated per neuron
    first = G.expected([cur], 50, 0.0, 0.95, 2, False)[0]
    v, rr, sc = first.v, first.r, first.spikes.copy()
    assert r.voltages().view(np.uint32).tolist() == v.tolist()
    for _ in range(2):
        r.simulate_spikes_auto()
        nv, nr = np.zeros_like(v), np.zeros_like(rr)
        for i in range(cur.size):
            a, b, s = cbind.lif(int(cur[i]), 50, 0.0, 0.95, 2, False, G.bits_f32(v[i]),
                                int(rr[i]), 0)
            nv[i], nr[i] = G.f32_bits(a), b
            sc[i] += s
        v, rr = nv, nr
        assert r.voltages().view(np.uint32).tolist() == v.tolist()
        assert r.refractory().tolist() == rr.tolist()
        assert r.spike_counts().tolist() == sc.tolist()
        assert r.total_spikes == int(sc.sum())
