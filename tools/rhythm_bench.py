"""Beat classes on the device: what `BeatClassifier.classify` and `BeatClassPool.push` cost.

Two legs:
  records  `BeatClassifier.classify` at the detector's peaks on `--shapes` (default 64x12x648000 and 64x2x648000: records x leads
           x samples, 30 minutes at 360 Hz): ms per call (device events around `--reps` calls after `--warm`, the median), beats/s,
           and GB/s against the bytes the definition has to move - a beat's extended window once and the windows of its up to 8
           neighbours, 4 leads beats (2 (Wb + Sa) + 1 + 8 (2 Wb + 1)) bytes, most of which the cache serves - as a fraction of
           `--hbm-peak` (GB/s; the MI355X's 8000).  The detection itself is timed beside it (`detect_ms`).
  pool     `BeatClassPool.push` with `--streams` streams, one second of samples per stream and call: median / p99 ms per push
           (host clock around the call, which synchronises), after `--warm` calls and once every stream has given nine beats;
           beside it the same pushes into a `BeatPool` alone (`detect_push_median_ms`).

Prints one JSON line.  Needs a HIP device: there is no fallback.

    python tools/rhythm_bench.py [--shapes 64x12x648000,64x2x648000] [--fs 360] [--streams 64] [--leads 2] [--reps 10] [--warm 3]
                                 [--calls 40] [--legs records,pool]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ecg_denoise_amd import BeatClassifier, BeatClassPool, BeatDetector, BeatPool, beat_latency, rhythm_geometry, synth  # noqa: E402

DEV = "cuda:0"


def _records(R, leads, T, distinct=4):
    base = torch.tensor(synth.make_records_with_rhythm(min(R, distinct), leads, T, seed=5)[0], device=DEV)
    return base.repeat(-(-R // base.shape[0]), 1, 1)[:R].contiguous()


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


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
    return _median(ts), ts


def records_leg(args, R, leads, T):
    x = _records(R, leads, T)
    det, cls = BeatDetector(args.fs, device=DEV), BeatClassifier(args.fs, device=DEV)
    beats = det.detect(x)
    ms, all_ms = _event_ms(lambda: cls.classify(x, beats), args.reps, args.warm)
    dms, _ = _event_ms(lambda: det.detect(x), max(2, args.reps // 2), 1)
    c = cls.classify(x, beats)
    n = int(beats.count.sum())
    g = rhythm_geometry(args.fs)
    nbytes = 4 * leads * n * (2 * (g["Wb"] + g["Sa"]) + 1 + 8 * (2 * g["Wb"] + 1))
    return {"R": R, "leads": leads, "T": T, "fs": args.fs, "beats": n, "classify_ms": ms, "classify_ms_all": all_ms,
            "detect_ms": dms, "beats_per_s": n / ms * 1e3, "bytes": nbytes, "GB_per_s": nbytes / ms / 1e6,
            "hbm_fraction": nbytes / ms / 1e6 / args.hbm_peak,
            "classes": dict(zip(("N", "V", "S", "unclassified"), c.counts().sum(0).tolist()))}


def pool_leg(args):
    fs, S = args.fs, args.streams
    secs = args.warm + args.calls + int(np.ceil(beat_latency(fs))) + 20          # (nine beats at 50 bpm take 11 s)
    x = _records(min(S, 4), args.leads, secs * fs)
    out = {}
    for name, pool in (("push", BeatClassPool(args.leads, S, fs, device=DEV)), ("detect_push", BeatPool(args.leads, S, fs, device=DEV))):
        sids = [pool.open() for _ in range(S)]
        ts, beats = [], 0
        for i in range(secs):
            chunks = {sid: x[s % x.shape[0], :, i * fs:(i + 1) * fs] for s, sid in enumerate(sids)}
            t0 = time.perf_counter()
            res = pool.push(chunks)
            dt = time.perf_counter() - t0
            if i >= secs - args.calls:
                ts.append(1e3 * dt)
                beats += sum(len(v[0]) if isinstance(v, tuple) else len(v) for v in res.values())
        out[name + "_median_ms"] = _median(ts)
        out[name + "_p99_ms"] = sorted(ts)[max(0, -(-99 * len(ts) // 100) - 1)]
        out[name + "_beats"] = beats
    out.update(S=S, leads=args.leads, fs=fs, chunk=fs, calls=args.calls, times_real_time=1e3 / out["push_median_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x12x648000,64x2x648000")
    ap.add_argument("--fs", type=int, default=360)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--leads", type=int, default=2, help="leads of the pool leg")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--hbm-peak", type=float, default=8000.0, help="GB/s")
    ap.add_argument("--legs", default="records,pool")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rhythm_bench: needs a HIP device")
    res = {"tool": "rhythm_bench", "geometry": rhythm_geometry(args.fs)}
    if "records" in args.legs:
        res["records"] = []
        for shape in [s for s in args.shapes.split(",") if s]:
            R, leads, T = (int(v) for v in shape.split("x"))
            res["records"].append(records_leg(args, R, leads, T))
            torch.cuda.empty_cache()
    if "pool" in args.legs:
        res["pool"] = pool_leg(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
