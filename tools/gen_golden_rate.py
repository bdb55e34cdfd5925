"""Writes tests/golden/g9_rate.npz: what scipy.signal.resample_poly(x, up, down, window=('kaiser', 5.0), padtype='edge') gives
for the rate pairs and record lengths of tests/rate_util.py, and the filter bank of every pair.  Needs scipy (written with
1.15.3); the tests read the file and never import scipy.

    python tools/gen_golden_rate.py

Per case (fs_in, fs_out, T):  x_<fs_in>_<fs_out>_<T>  int16 (2, T)      seeded ADC-like records (rate_util.adc_records; whole
                                                                          numbers, so int16 holds them exactly)
                              y_<fs_in>_<fs_out>_<T>  fp64  (2, T_out)   scipy's result for them as fp64
Per pair:                     bank_<fs_in>_<fs_out>   fp64  (half + 1,)  the first half + 1 of the 2 half + 1 taps
                                                                          (firwin(...) * up as resample_poly forms it; the
                                                                          filter is symmetric, the other half mirrors it)
Two rows per case and half a bank per pair keep the file under 256 KB."""
import os
import sys

import numpy as np
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rate_util as U  # noqa: E402


def main():
    out = {}
    for fi, fo in U.PAIRS:
        up, down = U.ratio(fi, fo)
        half = 10 * max(up, down)
        h = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
        assert np.max(np.abs(h - h[::-1])) <= 1e-16 * np.max(np.abs(h)) * 4, (fi, fo)
        out[f"bank_{fi}_{fo}"] = h[:half + 1]
        for T in U.LENGTHS[(fi, fo)]:
            x = U.adc_records(1, U.LEADS, T, seed=fi * 10000 + fo + T)[0]
            assert np.all(x == x.astype(np.int16))
            y = signal.resample_poly(x, up, down, axis=-1, window=("kaiser", 5.0), padtype="edge")
            assert y.dtype == np.float64 and y.shape == (U.LEADS, U.length(T, up, down)), (y.dtype, y.shape)
            out[f"x_{fi}_{fo}_{T}"] = x.astype(np.int16)
            out[f"y_{fi}_{fo}_{T}"] = y
    path = os.path.join(ROOT, "tests", "golden", "g9_rate.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
