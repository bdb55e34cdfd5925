"""Writes tests/golden/g10_fft.npz: the designed inputs of tests/fft_util.py at L in {16, 30, 112, 1000} (2 items of 3 leads
with amplitudes 1, 0.3, 0.02, threshold 0.04), what the fp64 restatement `fft_util.fft_denoise_ref` gives for them, and the
kept counts.  numpy only (written with the version the file records).  The file pins the RESTATEMENT: the reference's
`fft_denoise` (local_utils/denoisefunc.py:36-66) cannot run - it never imports `fft` / `ifft` - so no golden can come from it.

    python tools/gen_golden_fft.py

Per L:  x_<L>  fp32 (2, 3, L)   y_<L>  fp64 (2, 3, L)   kept_<L>  int64 (2,)   margin_<L>  fp64 (2,)
and, from the same inputs taken as 6 independent rows,  y2_<L>  fp64 (6, L)   kept2_<L>  int64 (6,)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fft_util as U  # noqa: E402


def main():
    out = {"numpy_version": np.array(np.__version__), "threshold": np.array(U.THRESHOLD)}
    for L in U.GOLDEN_LENGTHS:
        x = U.designed(U.GOLDEN_GROUPS, U.GOLDEN_AMPS, L, seed=1000 + L)
        y, kept, margin = U.fft_denoise_ref(x)
        y2, kept2, _ = U.fft_denoise_ref(x.reshape(-1, L))
        assert margin.min() >= 1e-2, (L, margin)
        out[f"x_{L}"], out[f"y_{L}"], out[f"kept_{L}"], out[f"margin_{L}"] = x, y, kept, margin
        out[f"y2_{L}"], out[f"kept2_{L}"] = y2, kept2
    path = os.path.join(ROOT, "tests", "golden", "g10_fft.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
