"""Injected-current cases for the LIF and top-N kernels -- TEST INFRASTRUCTURE ONLY.

The grid (PARAMS x STEPS x COUNTS x three rounds) and what the step-by-step
loop (cbind.lif: `steps` calls of LifNeuron::update, src/models.rs:34-51)
makes of it.  CPU only; tests/test_lif_grid.py checks that the grid reaches
every branch class of the closed form (neurokmer_amd/csrc/nk_device.h
lif_closed, nk_kernels.hip k_lif_apply / fresh_spikes), tests/test_gpu_lif.py
drives the kernels with it.
"""
from __future__ import annotations

import struct
from collections import namedtuple

import numpy as np

from . import cbind

INF, NAN = float("inf"), float("nan")

# (threshold, leak, refractory)
PARAMS = [
    (1.0, 0.95, 2),
    (0.5, 1.0, 0),
    (0.0, 0.95, 2),
    (1.0, 0.0, 5),
    (3.0, 0.99, 1),
    (1.0, 0.95, 1000),
    (1.0, -0.5, 1),
    (1.0, 1.5, 3),
    (-1.0, 0.9, 0),
    (INF, 0.9, 2),
    (NAN, 0.9, 2),
    (1.0, 0.95, 2**32 - 1),
    (1e-30, 0.5, 0),
    (16777216.0, 1.0, 0),
    (1.0, 0.999, 7),
]

STEPS = (1, 2, 3, 7, 1000, 1003, 20000)

COUNTS = (0, 1, 2, 3, 7, 49, 50, 51, 52, 53, 99, 100, 101, 999, 1000, 1001, 1999, 2000, 2001,
          3000, 65535, 65536, 65537, 2**24 - 1, 2**24, 2**24 + 1, 2**32 - 1, 2**32, 2**53 + 1,
          2**63, 2**64 - 1)

SHIFTS = (0, 5, 11)
TABLE_ROWS = 1 << 16  # the closed-form table of fresh neurons: counts below this

STATES = ("fresh", "carried")
SIZES = ("table", "past")  # count < TABLE_ROWS or not
SPIKING = ("none-stationary", "none-moving", "one-refractory", "one-r0", "several-refractory",
           "several-rest", "several-v")
KINDS = ("skipped", "drain") + SPIKING

# One round of expected(): the state every neuron entered with (v as u32 bits),
# the state it left with, its spike count so far and this round's spikes.
Round = namedtuple("Round", "v_in r_in v r spikes new")


def rounds(pool, shifts=SHIFTS):
    """Count vectors of length `pool`: COUNTS tiled, then rotated by each shift
    (neuron i sees COUNTS[(i + shift) % len(COUNTS)])."""
    c = np.array(COUNTS, dtype=np.uint64)
    i = np.arange(pool)
    return [c[(i + s) % len(COUNTS)] for s in shifts]


def f32_bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def bits_f32(b) -> float:
    return struct.unpack("<f", struct.pack("<I", int(b)))[0]


def _one(memo, count, vb, r, steps, thr, leak, refr, skip_zero):
    key = (count, vb, r, steps, skip_zero)
    got = memo.get(key)
    if got is None:
        v, r2, sp = cbind.lif(count, steps, thr, leak, refr, skip_zero, bits_f32(vb), r, 0)
        got = memo[key] = (f32_bits(v), r2, sp)
    return got


def expected(rounds_, steps, thr, leak, refr, streaming):
    """The step-by-step loop per neuron over the rounds, (v, r, spikes) carried
    from one round to the next -> a list of Round.  steps: one value, or one
    per round.  streaming: zero counts are stepped too (skip_zero off)."""
    per_round = [steps] * len(rounds_) if np.isscalar(steps) else list(steps)
    assert len(per_round) == len(rounds_)
    pool = len(rounds_[0])
    vb = np.zeros(pool, np.uint32)
    r = np.zeros(pool, np.uint32)
    sc = np.zeros(pool, np.uint64)
    memo = {}
    out = []
    for counts, st in zip(rounds_, per_round):
        counts = np.asarray(counts, np.uint64)
        state = np.stack([counts, vb.astype(np.uint64), r.astype(np.uint64)], axis=1)
        uniq, inv = np.unique(state, axis=0, return_inverse=True)
        res = np.array([_one(memo, int(c), int(b), int(x), int(st), thr, leak, refr,
                             not streaming) for c, b, x in uniq], dtype=np.uint64).reshape(-1, 3)
        res = res[np.asarray(inv).reshape(-1)]
        new = res[:, 2].copy()
        sc = sc + new
        out.append(Round(vb, r, res[:, 0].astype(np.uint32), res[:, 1].astype(np.uint32), sc, new))
        vb, r = out[-1].v, out[-1].r
    return out


def top_rows(spikes, n):
    """top_abundant_neurons(n) of these spike counts with no input counted:
    (index, spikes, 0) by spikes descending, index ascending."""
    spikes = np.asarray(spikes, np.uint64)
    idx = np.arange(spikes.size)
    order = np.lexsort((idx, np.iinfo(np.uint64).max - spikes))[:min(n, spikes.size)]
    return [(int(i), int(spikes[i]), 0) for i in order]


def current(count, steps) -> np.float32:
    """(count as f64 / steps as f64) as f32"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.float32(np.float64(count) / np.float64(steps))


def stationary(v_bits, leak, c) -> bool:
    """One more update leaves v as it is: f32(f32(v) * leak) + c == v, the two
    operations rounded to f32 separately."""
    v = np.float32(bits_f32(v_bits))
    with np.errstate(all="ignore"):
        t = np.float32(v * np.float32(leak))
        return bool(np.float32(t + c) == v)


def outcome(count, steps, thr, leak, refr, streaming, v_in, r_in, v_out, r_out, new):
    """(state, size, kind) of one (neuron, round) from oracle values alone
    (v_in / v_out: u32 bits)."""
    state = "fresh" if bits_f32(v_in) == 0.0 and r_in == 0 else "carried"
    size = "table" if count < TABLE_ROWS else "past"
    if count == 0 and not streaming:
        kind = "skipped"
    elif r_in >= steps:
        kind = "drain"
    elif new == 0:
        kind = "none-stationary" if stationary(v_out, leak, current(count, steps)) else "none-moving"
    elif new == 1:
        kind = "one-refractory" if r_out else "one-r0"
    elif r_out:
        kind = "several-refractory"
    else:
        kind = "several-rest" if bits_f32(v_out) == 0.0 else "several-v"
    return state, size, kind


def cost_fixed(cost) -> int:
    """Rust's `(cost * 1000.0) as u64`: saturating, NaN and negatives -> 0."""
    x = float(cost) * 1000.0
    if not x > 0.0:
        return 0
    if x >= 18446744073709551616.0:
        return 2**64 - 1
    return int(x)


def energy(total_spikes, cost) -> float:
    """EnergyTracker::total_energy after total_spikes spikes at `cost` each:
    the fixed-point sum wraps modulo 2^64 (src/models.rs:159-172)."""
    return float((int(total_spikes) * cost_fixed(cost)) % 2**64) / 1000.0
