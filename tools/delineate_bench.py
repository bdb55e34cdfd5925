"""Beat delineation on the device: what `BeatDelineator.delineate` costs.

`--shapes` (default 64x2x648000@360 and 16x12x900000@500: records x leads x samples @ rate, 30 minutes each) are synthetic rhythm
records (at most four distinct ones, repeated; the 500 Hz records are the same samples read at 500 Hz).  Per shape the beats are
the detector's; `delineate` is timed with device events around `--reps` calls after `--warm` (the median), and reported as ms
per call and beats/s, beside the detection (`detect_ms`) and how many beats got their QRS bounds and their QT.

Prints one JSON line.  Needs a HIP device: there is no fallback.

    python tools/delineate_bench.py [--shapes 64x2x648000@360,16x12x900000@500] [--reps 10] [--warm 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ecg_denoise_amd import BeatDelineator, BeatDetector, delineate_geometry, synth  # noqa: E402

DEV = "cuda:0"


def _records(R, leads, T, distinct=4):
    base = torch.tensor(synth.make_records_with_rhythm(min(R, distinct), leads, T, seed=5)[0], device=DEV)
    return base.repeat(-(-R // base.shape[0]), 1, 1)[:R].contiguous()


def _event_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2], ts


def leg(args, R, leads, T, fs):
    x = _records(R, leads, T)
    det, dl = BeatDetector(fs, device=DEV), BeatDelineator(fs, device=DEV)
    beats = det.detect(x)
    ms, all_ms = _event_ms(lambda: dl.delineate(x, beats), args.reps, args.warm)
    dms, _ = _event_ms(lambda: det.detect(x), max(2, args.reps // 2), 1)
    f = dl.delineate(x, beats)
    n = int(beats.count.sum())
    m = f.measurable()
    return {"R": R, "leads": leads, "T": T, "fs": fs, "geometry": delineate_geometry(fs), "beats": n, "cap": int(beats.peaks.shape[1]),
            "delineate_ms": ms, "delineate_ms_all": all_ms, "detect_ms": dms, "beats_per_s": n / ms * 1e3,
            "qrs_measured": int(m["qrs"].sum()), "qt_measured": int(m["qt"].sum()),
            "median_qrs_ms": float(f.qrs_ms().nanmedian()), "median_qt_ms": float(f.qt_ms().nanmedian())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x2x648000@360,16x12x900000@500")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("delineate_bench: needs a HIP device")
    res = {"tool": "delineate_bench", "legs": []}
    for shape in [s for s in args.shapes.split(",") if s]:
        dims, fs = shape.split("@")
        R, leads, T = (int(v) for v in dims.split("x"))
        res["legs"].append(leg(args, R, leads, T, int(fs)))
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
