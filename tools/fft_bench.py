"""Throughput of the FFT-threshold baseline (`fft_denoise`, ral_fft.hip) on one MI355X: device-event medians after a warm-up at

    (65536 rows, L = 256)   (16384 x 2, L = 1000)   (4096 x 12, L = 1024)   (2048 x 2, L = 8192)   (4096, L = 1008: direct path)

Per shape: ms per call, rows/s and algorithmic GB/s at 8 B per sample (a sample is read once and written once when the group is
resident; the two-pass form reads it twice, the figure still counts 8 B).  `wavelet_denoise` runs at the same shapes taken as
2-D rows (it takes even L <= 8192) as context.  The calls are timed through the public functions with device tensors, so a
call includes the allocation of its result.  One text line per shape and one JSON line at the end.

    python tools/fft_bench.py [--reps 20] [--warmup 3]            (writes nothing: redirect into profiles/fft_bench.txt)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ecg_denoise_amd import _lib, fft_denoise, wavelet_denoise  # noqa: E402

SHAPES = ((65536, 1, 256), (16384, 2, 1000), (4096, 12, 1024), (2048, 2, 8192), (4096, 1, 1008))


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fft_bench: needs a HIP device")
    g = torch.Generator().manual_seed(2023)
    out = []
    for groups, leads, L in SHAPES:
        x = torch.randn(groups, leads, L, generator=g).cuda()
        x = x.reshape(groups, L) if leads == 1 else x
        rows = groups * leads
        two_pass = _lib.lib().ral_fft_denoise_scratch_bytes(groups, leads, L) > 0
        row = {"groups": groups, "leads": leads, "L": L, "rows": rows, "launches": 3 if two_pass else 1}
        for name, fn in (("fft", lambda: fft_denoise(x)), ("wavelet", lambda: wavelet_denoise(x.reshape(rows, L)))):
            ms, lo, hi = median_ms(fn, args.reps, args.warmup)
            row[name] = {"ms": ms, "ms_min": lo, "ms_max": hi, "rows_per_s": rows / ms * 1e3, "GBps_at_8B_per_sample": 8 * rows * L / ms / 1e6}
        out.append(row)
        print(f"{groups:6d} x {leads:2d} x {L:5d}   fft {row['fft']['ms']:8.4f} ms  {row['fft']['rows_per_s']:12.0f} rows/s  "
              f"{row['fft']['GBps_at_8B_per_sample']:8.1f} GB/s   wavelet {row['wavelet']['ms']:8.4f} ms  "
              f"{row['wavelet']['rows_per_s']:12.0f} rows/s  {row['wavelet']['GBps_at_8B_per_sample']:8.1f} GB/s")
    print(json.dumps({"tool": "fft_bench", "reps": args.reps, "warmup": args.warmup, "shapes": out}))


if __name__ == "__main__":
    main()
