"""CPU-side checks of the 12-lead streaming entry points (ral_newrale_stream_front / _back): both are exported, and bad
arguments are refused with an error message before anything is launched (no GPU here: a launch would fail)."""
import ctypes as C

import numpy as np
import pytest

from ecg_denoise_amd import _lib

NAMES = ("ral_newrale_stream_front", "ral_newrale_stream_back")


def _buf(n):
    a = np.zeros(n, dtype=np.float32)
    return a, C.c_void_p(a.ctypes.data)


def test_symbols_exported():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name


# (R, T, L, hop, w0, nw): every case must be refused
BAD = {
    "T_shorter_than_L": (1, 1000, 1024, 1024, 0, 1),
    "odd_overlap": (1, 5000, 1024, 1023, 0, 1),
    "L_not_multiple_of_16": (1, 5000, 1000, 1000, 0, 1),
    "L_above_1024": (1, 5000, 1040, 1040, 0, 1),
    "L_zero": (1, 5000, 0, 0, 0, 1),
    "hop_zero": (1, 5000, 256, 0, 0, 1),
    "hop_above_L": (1, 5000, 256, 258, 0, 1),
    "window_range_past_end": (2, 1024 * 3, 1024, 1024, 4, 3),     # n = 3 per record: windows [4, 7) of 6
    "negative_w0": (1, 5000, 256, 256, -1, 1),
    "no_windows": (1, 5000, 256, 256, 0, 0),
    "no_records": (0, 5000, 256, 256, 0, 1),
}


def _front(R, T, L, hop, w0, nw, ptrs):
    rec, prm, inner, stats = ptrs
    return _lib.lib().ral_newrale_stream_front(rec, R, T, L, hop, w0, nw, prm, inner, stats, None)


def _back(R, T, L, hop, w0, nw, ptrs):
    iy, stats, prm, out = ptrs
    return _lib.lib().ral_newrale_stream_back(iy, stats, prm, R, T, L, hop, w0, nw, out, None)


@pytest.mark.parametrize("which", ["front", "back"])
@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_are_refused(which, case):
    keep = [_buf(16) for _ in range(4)]            # valid host pointers; nothing may reach them
    ptrs = [p for _, p in keep]
    fn = _front if which == "front" else _back
    rc = fn(*BAD[case], ptrs)
    assert rc != 0, case
    msg = _lib.lib().ral_last_error().decode()
    assert f"newrale_stream_{which}" in msg and "need" in msg, msg


@pytest.mark.parametrize("which", ["front", "back"])
@pytest.mark.parametrize("null_at", range(4))
def test_null_pointers_are_refused(which, null_at):
    keep = [_buf(16) for _ in range(4)]
    ptrs = [p for _, p in keep]
    ptrs[null_at] = None
    fn = _front if which == "front" else _back
    assert fn(1, 5000, 256, 256, 0, 1, ptrs) != 0
    assert "null pointer" in _lib.lib().ral_last_error().decode()
