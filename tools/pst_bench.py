"""P wave and ST level on the device: what `PStMeasurer.measure` costs, beside `BeatDelineator.delineate`.

`--shapes` (default 64x2x648000@360 and 16x12x900000@500: records x leads x samples @ rate, 30 minutes each) are synthetic rhythm
records (at most four distinct ones, repeated; the 500 Hz records are the same samples read at 500 Hz).  Per shape the beats are
the detector's and the fiducials the delineator's; `measure` and `delineate` on the same records and beats are timed with device
events, alternating in one process (`--reps` pairs after `--warm`, the medians), and reported as ms per call and beats/s, beside
how many beats got a P wave and an ST level.

Prints one JSON line.  Needs a HIP device: there is no fallback.

    python tools/pst_bench.py [--shapes 64x2x648000@360,16x12x900000@500] [--reps 10] [--warm 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ecg_denoise_amd import BeatDelineator, BeatDetector, PStMeasurer, pst_geometry, synth  # noqa: E402

DEV = "cuda:0"


def _records(R, leads, T, distinct=4):
    base = torch.tensor(synth.make_records_with_rhythm(min(R, distinct), leads, T, seed=5)[0], device=DEV)
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
    dl, ms = BeatDelineator(fs, device=DEV), PStMeasurer(fs, device=DEV)
    beats = BeatDetector(fs, device=DEV).detect(x)
    f = dl.delineate(x, beats)
    for _ in range(args.warm):
        ms.measure(x, f), dl.delineate(x, beats)
    m_all, d_all = [], []
    for _ in range(args.reps):                                # alternating, one process
        m_all.append(_event_ms(lambda: ms.measure(x, f)))
        d_all.append(_event_ms(lambda: dl.delineate(x, beats)))
    mms, dms = sorted(m_all)[len(m_all) // 2], sorted(d_all)[len(d_all) // 2]
    pts = ms.measure(x, f)
    n = int(beats.count.sum())
    m = pts.measurable()
    st = pts.st[m["st"]]
    return {"R": R, "leads": leads, "T": T, "fs": fs, "geometry": pst_geometry(fs), "beats": n, "cap": int(beats.peaks.shape[1]),
            "measure_ms": mms, "measure_ms_all": m_all, "delineate_ms": dms, "delineate_ms_all": d_all,
            "measure_beats_per_s": n / mms * 1e3, "delineate_beats_per_s": n / dms * 1e3,
            "p_found": int(m["p"].sum()), "st_read": int(m["st"].sum()), "median_pr_ms": float(pts.pr_ms().nanmedian()),
            "median_p_ms": float(pts.p_ms().nanmedian()), "median_abs_st": float(st.abs().median()) if st.numel() else float("nan")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x2x648000@360,16x12x900000@500")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pst_bench: needs a HIP device")
    res = {"tool": "pst_bench", "legs": []}
    for shape in [s for s in args.shapes.split(",") if s]:
        dims, fs = shape.split("@")
        R, leads, T = (int(v) for v in dims.split("x"))
        res["legs"].append(leg(args, R, leads, T, int(fs)))
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
