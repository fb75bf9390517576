"""Records placed at tile, lane and chunk edges of the count kernels -- TEST
INFRASTRUCTURE ONLY.

Every count kernel stages its input through stage_tile / window_key*
(neurokmer_amd/csrc/nk_tile.h): tiles of 4096 (kTile) or 8192 (kPartTile)
k-mer start positions with a 64-base halo, 16 positions per lane, 16-byte
input chunks with a byte path for the input's last partial chunk, 32-position
words of the "window crosses a record end" mask.  The layouts here put record
ends, empty records, short records, invalid bytes and the end of the input at
fixed distances from those positions, so that no edge is left to where a random
layout happens to land.  CPU only; tests/test_tile_edges.py checks that the
layouts hold what they promise, tests/test_gpu_tile_edges.py drives the
kernels with them.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from neurokmer_amd import synth

TILE = 4096        # kTile: the direct-atomic and exact-table kernels
PART_TILE = 8192   # kPartTile: K1a and the generic / wide partition

EXTRAS = ("empties", "straddle", "single_before", "single_at")
# A copy of the bases around every edge, TWIN_SHIFT further on and inside one
# record, and of the input's last bases at END_TWIN past the last edge.  The
# uniques rescans use a window's key only to deduplicate: with every k-mer
# distinct a wrong key stays distinct and nothing changes; with a twin
# elsewhere, a wrong key at the edge no longer merges with its twin's.  A
# rescan that drops a window shows only where the window has no twin, so the
# uniques cases run the layouts with the twins and without.
TWIN_HALF, TWIN_SHIFT, TWIN_REC = 130, 2053, (1800, 2300)
END_TWIN, END_LEN, END_REC = 1000, 100, (900, 1200)


def deltas(k):
    """Distances from an edge at which edge_layout ends a record, deduplicated."""
    return sorted({-64, -k - 1, -k, -k + 1, -17, -16, -15, -1, 0, 1, 15, 16, 17, 31, 32, 33,
                   k - 2, k - 1, k, 63, 64, 65})


def edge_plan(k):
    """[(E, kind, boundaries)] of edge_layout(k, ...), E ascending: every
    multiple of 4096 inside the input with the record boundaries placed around
    it.  kind: a delta d (one record end at E + d) or one of EXTRAS:
      empties        three empty records whose offsets all equal E
      straddle       a record of length k - 1 that starts at E - (k - 1) // 2
      single_before  a record of length k whose one window starts at E - 1
      single_at      a record of length k whose one window starts at E
    The deltas go to the odd multiples of 4096 (edges of the 4096-position
    tiles only) and again to the even ones (edges of both tile sizes), then
    the extras to one edge of each parity."""
    plan = []
    for i, what in enumerate(list(deltas(k)) + list(EXTRAS)):
        for E in ((2 * i + 1) * TILE, (2 * i + 2) * TILE):
            if what == "empties":
                b = [E, E, E, E]
            elif what == "straddle":
                s = E - (k - 1) // 2
                b = [s, s + k - 1]
            elif what == "single_before":
                b = [E - 1, E - 1 + k]
            elif what == "single_at":
                b = [E, E + k]
            else:
                b = [E + what]
            plan.append((E, what, b))
    plan.sort(key=lambda t: t[0])
    return plan


def n_offsets(k):
    """dirty: one N per edge at E + one of these, cycling (47, 48, 63: the last
    two INV words of the 64-base halo)."""
    return (-1, 0, k - 1, k, 47, 48, 63)


def _n_at(E, k, i):
    return E + n_offsets(k)[i % 7]


def edge_layout(k, seed=1, dirty=False, twins=True):
    """-> (bases uint8, offs uint64[n_recs + 1]): random ACGT, a record end at
    every distance of deltas(k) from one odd and one even multiple of 4096,
    the EXTRAS, filler records of 200..3000 bases in between, with `twins` the
    twins (see TWIN_SHIFT; the offsets are the same without); the length is
    5 mod 16, so the input's last chunk takes
    stage_tile's byte path.
    dirty: an N at every edge (E + one of n_offsets(k), cycling), about 1 % of
    the bases in lower case, a few other IUPAC bytes."""
    plan = edge_plan(k)
    total = (len(plan) + 1) * TILE - 11
    rng = np.random.default_rng(1000 * seed + k)
    offs = [0]

    def fill_to(end):
        rem = end - offs[-1]
        assert rem >= 200, (offs[-1], end)
        while rem > 3000:
            L = int(rng.integers(200, min(3000, rem - 200) + 1))
            offs.append(offs[-1] + L)
            rem -= L
        offs.append(end)

    for E, _, b in plan:
        fill_to(b[0])
        offs.extend(b[1:])
        if E == plan[-1][0]:
            fill_to(E + END_REC[0])
            offs.append(E + END_REC[1])
        fill_to(E + TWIN_REC[0])
        offs.append(E + TWIN_REC[1])
    fill_to(total)
    bases = synth.random_bases(total, seed=synth.SEED + 7919 * seed + k)
    if dirty:
        lower = rng.random(total) < 0.01
        bases[lower] |= 0x20
        other = rng.integers(0, total, 24)
        bases[other] = np.frombuffer(b"RYKMSWBDHVn.-", np.uint8)[np.arange(24) % 13]
        for i, (E, _, _) in enumerate(plan):
            bases[_n_at(E, k, i)] = ord("N")
    if twins:
        for E, _, _ in plan:
            bases[E - TWIN_HALF + TWIN_SHIFT:E + TWIN_HALF + TWIN_SHIFT] = bases[E - TWIN_HALF:E + TWIN_HALF]
        last = plan[-1][0]
        bases[last + END_TWIN:last + END_TWIN + END_LEN] = bases[total - END_LEN:]
    return bases, np.array(offs, np.uint64)


def n_positions(k):
    """The positions edge_layout(k, dirty=True) overwrites with N."""
    return [_n_at(E, k, i) for i, (E, _, _) in enumerate(edge_plan(k))]


def truncate(bases, offs, n):
    """The first n bases: offsets clipped to n, records that start at or after
    n dropped (an empty input keeps one empty record)."""
    offs = np.asarray(offs, np.uint64)
    keep = int(np.searchsorted(offs[:-1], n, side="left"))  # records starting before n
    keep = max(keep, 1)
    o = np.minimum(offs[:keep + 1], np.uint64(n)).astype(np.uint64)
    return np.ascontiguousarray(bases[:n]), o


TAIL_T = (0, 4096, 8192, 16384)


def tail_r(k):
    return sorted({0, 1, k - 1, k, k + 1, 15, 16, 17, 31, 33})


def tail_inputs(k, twins=True):
    """[(T, r, bases, offs)]: inputs of T + r bases, a leading record of up to
    3 bases and one record with the rest.  T + r ends an input exactly on a
    tile edge (r = 0), leaves a last tile with fewer than k bases, and runs
    every n_bases mod 16 residue of interest through the byte path.  twins:
    the last 96 bases have a twin at base 1000 (T = 0: the bases repeat with
    period 3), so the last windows' keys matter to the uniques (see
    TWIN_SHIFT)."""
    out = []
    for T in TAIL_T:
        for r in tail_r(k):
            n = T + r
            if n == 0:
                continue
            lead = min(3, n - 1)
            bases = synth.random_bases(n, seed=synth.SEED + 31 * T + r + 1)
            if twins and T == 0:
                bases = np.resize(bases[:3], n)
            elif twins:
                bases[1000:1096] = bases[n - 96:]
            out.append((T, r, bases, np.array([0, lead, n], np.uint64)))
    return out


def many_records_tile(seed=5):
    """9000 records of one to three bases, then one of 5000 bases: the first
    8192-position tile holds more record ends than stage_tile's loop has
    threads (512), and so does the first 4096-position tile (256)."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([rng.integers(1, 4, 9000), [5000]])
    offs = np.zeros(lens.size + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    return synth.random_bases(int(offs[-1]), seed=synth.SEED + seed), offs


def n_kmers(offs, k):
    """sum(max(0, len - k + 1)) over the records."""
    lens = np.diff(np.asarray(offs, np.uint64).astype(np.int64))
    return int(np.clip(lens - k + 1, 0, None).sum())


# ---- the GPU cases (tests/test_gpu_tile_edges.py) ---------------------------
# path, environment, k values, key width, pool: one count path each
# (nk_count.cpp plan_count).  part-xcd: a canonical pool past 128 buckets takes
# the wide count with keys rolled in registers (gen_rolled64), a non-canonical
# one K1a with a sub-region per XCD; part-xcd-k1a keeps the canonical count on
# K1a too (NK_PART_BIG).
Row = namedtuple("Row", "path env ks width pool")
MATRIX = (
    Row("part-1", {}, (1, 15, 16, 17, 31, 32), 64, 5003),
    Row("part-many", {}, (16, 31, 32), 64, 2_000_003),
    Row("part-xcd", {}, (31,), 64, 16_000_000),
    Row("gen-compat", {}, (33, 63), 64, 100_003),
    Row("gen-128", {}, (33, 63, 64), 128, 100_003),
    Row("wide", {"NK_WIDE_BITS": "16"}, (31, 40), 64, 700_001),
    Row("wide-128", {"NK_WIDE_BITS": "17"}, (63,), 128, 700_001),
    Row("atomic", {"NK_FORCE_ATOMIC": "1"}, (16, 31, 40, 65), 64, 5003),
    Row("atomic-128", {"NK_FORCE_ATOMIC": "1"}, (17, 64), 128, 5003),
)
Case = namedtuple("Case", "path env k width canon dirty pool twins", defaults=(True,))


def path_cases():
    """Every MATRIX row at each of its k: canonical on the clean and the dirty
    layout, non-canonical (pack_kmer: the INV words, the raw bytes) on the
    dirty one."""
    out = [Case(r.path, r.env, k, r.width, canon, dirty, r.pool)
           for r in MATRIX for k in r.ks
           for canon, dirty in ((True, False), (True, True), (False, True))]
    out += [Case("part-xcd-k1a", {"NK_PART_BIG": "1"}, 31, 64, True, dirty, 16_000_000)
            for dirty in (False, True)]
    return out


def case_id(c):
    return (f"{c.path}-k{c.k}-{'canon' if c.canon else 'packed'}-{'dirty' if c.dirty else 'clean'}"
            f"{'' if c.twins else '-notwins'}")


# The uniques of a top row come from a rescan with edge code of its own
# (k_uniq_scan re-keys a kept record from global memory, with a byte path of
# its own at the end of the input; k_uniq_lanes rolls a lane's bytes;
# k_uniq_gen and the direct-atomic kernels stage the tile again), and only
# windows of top rows reach it: 20 rows of 5003 are 0.4 % of the windows.  With
# every neuron a top row (pool <= the 1024 rows a handle selects) every window
# of the layout goes through the rescan of its path.
UNIQ_POOL = 1021
UNIQ_ROWS = (
    Row("part", {}, (16, 31, 32), 64, UNIQ_POOL),
    Row("gen-compat", {}, (40, 63), 64, UNIQ_POOL),
    Row("gen-128", {}, (33, 64), 128, UNIQ_POOL),
    Row("wide", {"NK_WIDE_BITS": "16"}, (31, 40), 64, UNIQ_POOL),
    Row("wide-128", {"NK_WIDE_BITS": "17"}, (63,), 128, UNIQ_POOL),
    Row("atomic", {"NK_FORCE_ATOMIC": "1"}, (31, 65), 64, UNIQ_POOL),
    Row("atomic-128", {"NK_FORCE_ATOMIC": "1"}, (64,), 128, UNIQ_POOL),
)


def uniq_cases():
    return [Case(r.path, r.env, k, r.width, canon, dirty, r.pool, twins)
            for r in UNIQ_ROWS for k in r.ks for canon, dirty in ((True, False), (False, True))
            for twins in (True, False)]


# (k, width, canon, pool) with exact_counts=True
EXACT_CASES = ((31, 64, True, 5003), (32, 64, False, 5003), (21, 64, True, 2_000_003),
               (63, 128, True, 5003))

# tails: (k, width, environment, canon, pool).  K1a and the direct-atomic
# kernels, the compat keys, 128-bit keys; the last three clip the lane's
# windows at the end of the input in code of their own (nk_wide.hip
# gen_rolled64, gen_rolled128 with k at compile time and at run time).  The
# handles select min(pool, 1024) rows: at UNIQ_POOL the uniques rescans see
# every window of every tail too.
TAIL_CONFIGS = tuple((k, 64, env, canon, UNIQ_POOL) for k in (1, 16, 31, 32)
                     for env in ({}, {"NK_FORCE_ATOMIC": "1"}) for canon in (True, False)) + \
    ((33, 64, {}, True, UNIQ_POOL), (33, 64, {}, False, UNIQ_POOL),
     (64, 128, {}, True, UNIQ_POOL), (64, 128, {}, False, UNIQ_POOL),
     (63, 128, {}, True, UNIQ_POOL), (31, 64, {"NK_WIDE_BITS": "16"}, True, 700_001))

# cuts (accumulate_device_from): first_pos = q + j.  (k, width, environment,
# pool): K1a's lane clip, window_valid (Gen, compat keys), and the lane clips
# of gen_rolled64 (wide, k <= 32) and gen_rolled128 (128-bit keys, k > 48)
CUT_CONFIGS = ((31, 64, {}, 100_003), (40, 64, {}, 100_003),
               (31, 64, {"NK_WIDE_BITS": "16"}, 700_001), (63, 128, {}, 100_003))
CUT_J = (0, 1, 15, 16, 17, -1)


def all_ks():
    return sorted({k for r in MATRIX + UNIQ_ROWS for k in r.ks} | {c[0] for c in EXACT_CASES} |
                  {c[0] for c in TAIL_CONFIGS} | {c[0] for c in CUT_CONFIGS} | {5})


def cut_bases(k):
    """The two q of the cut test on edge_layout(k): a 16-aligned position in
    the middle of a tile, and an edge of both tile sizes; both at least 34
    bases into a record that goes on for 200 more (first_pos - 1 ..
    first_pos + 17 stay past the 32-base warm-up of the k > 32 compat keys
    and well inside the record)."""
    bases, offs = edge_layout(k)
    o = offs.astype(np.int64)
    out = []
    for want_edge in (False, True):
        for E in range(PART_TILE, int(o[-1]) - PART_TILE, PART_TILE):
            q = E if want_edge else E + 1920
            r = int(np.searchsorted(o, q, side="right")) - 1
            if q - o[r] >= 34 and o[r + 1] - q >= 200:
                out.append(q)
                break
    assert len(out) == 2
    return out
