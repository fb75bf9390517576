"""Argument checks of the enumeration entry points (include/neurokmer.h:
nk_export_counts_device, nk_export_counts, nk_count_spectrum) that need no
device: a null handle, and nk_count_spectrum's n_bins range, which is checked
before the handle is looked at."""
import ctypes as C

import numpy as np

from neurokmer_amd import _lib


def test_null_handle_is_invalid():
    L = _lib.load(share_torch=False)
    kp, cp, n = C.c_void_p(), C.c_void_p(), C.c_size_t(7)
    assert L.nk_export_counts_device(None, 1, 10, C.byref(kp), C.byref(cp), C.byref(n),
                                     None) == _lib.NK_E_INVALID
    assert "null counter" in _lib.last_error()
    keys, cnt = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    assert L.nk_export_counts(None, 1, 10, keys.ctypes.data, cnt.ctypes.data, 4) == _lib.NK_E_INVALID
    assert "null counter" in _lib.last_error()
    assert L.nk_export_counts(None, 1, 10, None, None, 0) == _lib.NK_E_INVALID
    hist = np.full(64, 9, np.uint64)
    assert L.nk_count_spectrum(None, hist.ctypes.data, 64) == _lib.NK_E_INVALID
    assert "null counter" in _lib.last_error()
    assert (hist == 9).all() and not keys.any()  # nothing written


def test_spectrum_bin_range_is_checked_first():
    L = _lib.load(share_torch=False)
    hist = np.zeros(4, np.uint64)
    for n_bins in (0, 1, 2**20 + 1):
        assert L.nk_count_spectrum(None, hist.ctypes.data, n_bins) == _lib.NK_E_INVALID
        assert "n_bins" in _lib.last_error()
    for n_bins in (2, 2**20):  # in range: the next check (the handle) answers
        assert L.nk_count_spectrum(None, hist.ctypes.data, n_bins) == _lib.NK_E_INVALID
        assert "null counter" in _lib.last_error()
