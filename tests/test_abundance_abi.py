"""What of the read abundance query (include/neurokmer.h: nk_query_abundance,
nk_query_abundance_device) can be checked without a device: the null-handle
check comes before anything that touches one, and the Python mirrors of
nk_read_stats and of the header's constants agree with the header."""
import ctypes as C
import os
import re

import numpy as np

from neurokmer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_handle_is_invalid_and_writes_nothing():
    L = _lib.load(share_torch=False)
    bases = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGT", np.uint8)
    offs = np.array([0, bases.size], np.uint64)
    cov = np.full(bases.size, 0xABCD, np.uint32)
    stats = np.full(40, 0x5A, np.uint8)
    assert L.nk_query_abundance(None, bases.ctypes.data, offs.ctypes.data, 1, 1, cov.ctypes.data,
                                stats.ctypes.data) == _lib.NK_E_INVALID
    assert "null counter" in _lib.last_error()
    assert L.nk_query_abundance_device(None, bases.ctypes.data, offs.ctypes.data, 1, bases.size, 1,
                                       cov.ctypes.data, stats.ctypes.data,
                                       None) == _lib.NK_E_INVALID
    assert "null counter" in _lib.last_error()
    assert L.nk_query_abundance(None, None, None, 0, 0, None, None) == _lib.NK_E_INVALID
    assert "null counter" in _lib.last_error()
    assert (cov == 0xABCD).all() and (stats == 0x5A).all()


def test_read_stats_layout():
    assert C.sizeof(_lib.NkReadStats) == 40
    dt = _lib.read_stats_dtype()
    assert dt.itemsize == 40
    want = {"n_kmers": (0, 8), "n_present": (8, 8), "sum": (16, 8), "min": (24, 4),
            "max": (28, 4), "median": (32, 4), "_pad": (36, 4)}
    assert set(dt.names) == set(want)
    for name, (off, size) in want.items():
        field = getattr(_lib.NkReadStats, name)
        assert (field.offset, field.size) == (off, size), name
        assert dt.fields[name][1] == off and dt.fields[name][0].itemsize == size, name
        assert dt.fields[name][0].kind == "u", name
    # one row written through ctypes reads back through numpy
    row = _lib.NkReadStats(7, 5, 2**40 + 3, 1, 900, 12, 0)
    a = np.frombuffer(bytes(row), dt)
    assert (int(a["n_kmers"][0]), int(a["n_present"][0]), int(a["sum"][0]), int(a["min"][0]),
            int(a["max"][0]), int(a["median"][0])) == (7, 5, 2**40 + 3, 1, 900, 12)


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "neurokmer.h")).read()
    defs = dict(re.findall(r"#define\s+(NK_COV_NONE|NK_QUERY_[A-Z_]+)\s+(0x[0-9A-Fa-f]+|\d+)", text))
    assert int(defs["NK_COV_NONE"], 0) == _lib.NK_COV_NONE == 2**32 - 1
    assert int(defs["NK_QUERY_WAVE_MAX"], 0) == _lib.NK_QUERY_WAVE_MAX
    assert int(defs["NK_QUERY_BLOCK_MAX"], 0) == _lib.NK_QUERY_BLOCK_MAX
    assert 64 <= _lib.NK_QUERY_WAVE_MAX < _lib.NK_QUERY_BLOCK_MAX
