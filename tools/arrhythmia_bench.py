"""Rhythm findings on the device: what `ArrhythmiaAnalyzer.analyse` costs, alone and as the last of the five calls detect ->
classify -> delineate -> P / ST -> analyse.

`--shapes` (default 64x2x648000@360 and 16x12x900000@500: records x leads x samples @ rate, 30 minutes each) are synthetic records
with one episode of atrial fibrillation each (`synth.make_records_with_af`; at most four distinct ones, repeated; the 500 Hz
records are the same samples read at 500 Hz).  Per shape the beats are the detector's, the labels the classifier's and the P input
the delineator's and the P / ST measurement's; `analyse` on them and the whole chain on the records are timed with device events,
alternating in one process (`--reps` pairs after `--warm`, the medians), and reported as ms per call, windows/s and records/s,
beside how many windows got each flag.  There is no target.

Prints one JSON line.  Needs a HIP device: there is no fallback.

    python tools/arrhythmia_bench.py [--shapes 64x2x648000@360,16x12x900000@500] [--reps 10] [--warm 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ecg_denoise_amd import (ArrhythmiaAnalyzer, BeatClassifier, BeatDelineator, BeatDetector, PStMeasurer, synth)  # noqa: E402
from ecg_denoise_amd.arrhythmia import FLAGS  # noqa: E402

DEV = "cuda:0"


def _records(R, leads, T, distinct=4):
    base = torch.tensor(synth.make_records_with_af(min(R, distinct), leads, T, seed=5)[0], device=DEV)
    return base.repeat(-(-R // base.shape[0]), 1, 1)[:R].contiguous()


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def leg(args, R, leads, T, fs):
    x = _records(R, leads, T)
    det, cls = BeatDetector(fs, device=DEV), BeatClassifier(fs, device=DEV)
    dl, ms, ana = BeatDelineator(fs, device=DEV), PStMeasurer(fs, device=DEV), ArrhythmiaAnalyzer(fs, device=DEV)

    def chain():
        beats = det.detect(x)
        return ana.analyse(beats, T, cls.classify(x, beats), ms.measure(x, dl.delineate(x, beats)))

    beats = det.detect(x)
    classes, pst = cls.classify(x, beats), ms.measure(x, dl.delineate(x, beats))
    for _ in range(args.warm):
        ana.analyse(beats, T, classes, pst), chain()
    a_all, c_all = [], []
    for _ in range(args.reps):                                # alternating, one process
        a_all.append(_event_ms(lambda: ana.analyse(beats, T, classes, pst)))
        c_all.append(_event_ms(chain))
    ams, cms = sorted(a_all)[len(a_all) // 2], sorted(c_all)[len(c_all) // 2]
    rh = ana.analyse(beats, T, classes, pst)
    g = {k: v for k, v in ana.geometry.items() if k != "fs"}
    return {"R": R, "leads": leads, "T": T, "fs": fs, "geometry": g, "beats": int(beats.count.sum()), "cap": int(beats.peaks.shape[1]),
            "windows": len(rh), "analyse_ms": ams, "analyse_ms_all": a_all, "chain_ms": cms, "chain_ms_all": c_all,
            "analyse_windows_per_s": len(rh) / ams * 1e3, "analyse_records_per_s": R / ams * 1e3,
            "chain_windows_per_s": len(rh) / cms * 1e3, "chain_records_per_s": R / cms * 1e3,
            "flagged": {k: int(rh.flag(k).sum()) for k in FLAGS}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x2x648000@360,16x12x900000@500")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("arrhythmia_bench: needs a HIP device")
    res = {"tool": "arrhythmia_bench", "legs": []}
    for shape in [s for s in args.shapes.split(",") if s]:
        dims, fs = shape.split("@")
        R, leads, T = (int(v) for v in dims.split("x"))
        res["legs"].append(leg(args, R, leads, T, int(fs)))
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
