"""CPU-side checks of live 12-lead streaming (NewRALELiveDenoiser; ral_newrale_live_front / ral_newrale_live_back): the entry
points and the class are exported, and bad arguments and null pointers are refused with a message before anything is launched
(no GPU here: a launch would fail)."""
import ctypes as C

import numpy as np
import pytest

from ecg_denoise_amd import _lib

NAMES = ("ral_newrale_live_front", "ral_newrale_live_back")


def _buf(n):
    a = np.zeros(n, dtype=np.float32)
    return a, C.c_void_p(a.ctypes.data)


def test_symbols_exported():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name


def test_class_exported():
    import ecg_denoise_amd
    from ecg_denoise_amd.infer import NewRALELiveDenoiser
    assert ecg_denoise_amd.NewRALELiveDenoiser is NewRALELiveDenoiser


# ---- argument validation ----------------------------------------------------------------------------------------------
GOOD = dict(S=2, L=256, hop=256, C=256, base=0, k0=1, nw=1, T=-1, w0=0, nb=2)

# every case must be refused by both entry points (a bad window range, stream geometry or batch)
BAD_BOTH = {
    "no_streams": dict(S=0),
    "L_not_multiple_of_16": dict(L=250, hop=250),
    "L_above_1024": dict(L=1040, hop=1040),
    "L_zero": dict(L=0, hop=0),
    "hop_zero": dict(hop=0),
    "hop_above_L": dict(hop=258),
    "odd_overlap": dict(hop=255),
    "T_shorter_than_L": dict(T=200),
    "T_zero": dict(T=0),
    "k0_past_stream_end": dict(T=512, k0=2),           # a closed stream of 512 samples has windows 0 and 1
    "negative_k0": dict(k0=-1),
    "negative_w0": dict(w0=-1),
    "window_range_past_end": dict(w0=1, nb=2),          # w0 + nb > S * nw = 2
    "negative_nw": dict(nw=-1),
}
BAD_FRONT = {
    "window_before_history": dict(base=300),            # window 1 starts at 256, V at 300
    "window_past_chunk": dict(k0=1, nw=2),              # window 2 ends at 768, V = [0, 512)
    "negative_chunk": dict(C=-1),
    "nothing_to_do": dict(nb=0, hist_out=False),
    "history_in_place": dict(hist_out="hist"),
}
BAD_BACK = {
    "negative_lo": dict(lo=-1),
    "negative_m": dict(m=-1),
    "no_windows": dict(nb=0),
    "last_y_without_last_stats": dict(last="y"),
    "last_stats_without_last_y": dict(last="stats"),
}


def _front(a, ptrs):
    hist, x, hist_out, prm, inner, stats = ptrs
    ho = a.get("hist_out", True)
    ho = hist if ho == "hist" else (hist_out if ho else None)
    return _lib.lib().ral_newrale_live_front(hist, x, ho, a["S"], a["L"], a["hop"], a["C"], a["base"], a["k0"], a["nw"], a["T"],
                                             a["w0"], a["nb"], prm, inner, stats, None)


def _back(a, ptrs):
    iy, stats, prm, out, last_y, last_stats = ptrs
    last = a.get("last", "both")
    return _lib.lib().ral_newrale_live_back(iy, stats, prm, a["S"], a["L"], a["hop"], a["k0"], a["nw"], a["T"], a["w0"], a["nb"],
                                            a.get("lo", 0), a.get("m", 256), out, last_y if last in ("both", "y") else None,
                                            last_stats if last in ("both", "stats") else None, None)


CASES = [("front", c, v) for c, v in {**BAD_BOTH, **BAD_FRONT}.items()] + \
        [("back", c, v) for c, v in {**BAD_BOTH, **BAD_BACK}.items()]


@pytest.mark.parametrize("which,case,over", CASES, ids=[f"{w}-{c}" for w, c, _ in CASES])
def test_bad_arguments_are_refused(which, case, over):
    keep = [_buf(16) for _ in range(6)]            # valid host pointers; nothing may reach them
    ptrs = [p for _, p in keep]
    fn = _front if which == "front" else _back
    rc = fn({**GOOD, **over}, ptrs)
    assert rc != 0, case
    msg = _lib.lib().ral_last_error().decode()
    assert f"newrale_live_{which}" in msg and "need" in msg, msg


@pytest.mark.parametrize("which,null_at", [("front", i) for i in (0, 1, 3, 4, 5)] + [("back", i) for i in range(4)])
def test_null_pointers_are_refused(which, null_at):
    keep = [_buf(16) for _ in range(6)]
    ptrs = [p for _, p in keep]
    ptrs[null_at] = None
    fn = _front if which == "front" else _back
    assert fn(dict(GOOD), ptrs) != 0
    assert f"newrale_live_{which}: null pointer" in _lib.lib().ral_last_error().decode()
