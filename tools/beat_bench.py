"""Beat detection on the device: what `BeatDetector.detect` and `BeatPool.push` cost.

Two legs:
  records  `BeatDetector.detect` on `--records` x `--leads` x `--minutes` records at `--fs` (default 64 x 2 x 30 minutes at 360 Hz
           = 648 000 samples): ms per call (device events around `--reps` calls after `--warm`, the median), samples/s, and GB/s
           against the bytes the definition has to move - x once in, f and m once out and once in, 4 R T (leads + 4) bytes - as
           a fraction of `--hbm-peak` (GB/s; the MI355X's 8000).  Beside it the same pipeline written with torch ops on the
           same device (`conv1d` on edge-padded leads, squares summed over the leads, `avg_pool1d`, `max_pool1d` for the
           threshold window and the refractory rule, `max_pool1d(return_indices)` for the refinement, `nonzero`): its ms and the
           ratio.  The torch pipeline treats ties in the refractory rule symmetrically and pads the moving mean differently in
           no way that matters for time; `agree` is the share of records on which the two give the same list.
  pool     `BeatPool.push` with `--streams` streams, one second of samples per stream and call: median / p99 ms per push (host
           clock around the call, which synchronises), after `--warm` calls and once every stream is past the detector's latency.

Prints one JSON line.  Needs a HIP device: there is no fallback.

    python tools/beat_bench.py [--records 64] [--leads 2] [--minutes 30] [--fs 360] [--streams 64] [--reps 10] [--warm 3]
                               [--calls 40] [--no-torch]
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
import torch.nn.functional as F  # noqa: E402

from ecg_denoise_amd import BeatDetector, BeatPool, beat_bank, beat_geometry, beat_latency, synth  # noqa: E402

DEV = "cuda:0"


def _records(R, leads, T, distinct=4):
    base = torch.tensor(synth.make_records(min(R, distinct), leads, T, seed=5), device=DEV)
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


def torch_detect(x, fs, alpha=0.35, floor=0.0):
    """the detector's pipeline in torch ops -> [peaks of each record] (device tensors)"""
    g = beat_geometry(fs)
    R, leads, T = x.shape
    h = torch.tensor(beat_bank(fs).astype(np.float32), device=x.device)
    xp = F.pad(x.reshape(R * leads, 1, T), (g["half"], g["half"]), mode="replicate")
    y = F.conv1d(xp, h.flip(0).view(1, 1, -1)).view(R, leads, T)
    f = (y * y).sum(1, keepdim=True)
    m = F.avg_pool1d(f, 2 * g["Wi"] + 1, 1, g["Wi"], count_include_pad=True)
    thr = torch.clamp(alpha * F.max_pool1d(m, 2 * g["Wt"] + 1, 1, g["Wt"]), min=floor)
    cand = (m > 0) & (m >= thr) & (m >= F.max_pool1d(m, 2 * g["Rf"] + 1, 1, g["Rf"]))
    _, top = F.max_pool1d(f, 2 * g["Rw"] + 1, 1, g["Rw"], return_indices=True)
    at = cand[:, 0].nonzero()
    peaks = top[at[:, 0], 0, at[:, 1]]
    return [peaks[at[:, 0] == r] for r in range(R)]


def records_leg(args):
    T = int(args.minutes * 60 * args.fs)
    x = _records(args.records, args.leads, T)
    det = BeatDetector(args.fs, device=DEV)
    ms, all_ms = _event_ms(lambda: det.detect(x), args.reps, args.warm)
    nbytes = 4 * args.records * T * (args.leads + 4)
    b = det.detect(x)
    leg = {"R": args.records, "leads": args.leads, "T": T, "fs": args.fs, "detect_ms": ms, "detect_ms_all": all_ms,
           "samples_per_s": args.records * T / ms * 1e3, "bytes": nbytes, "GB_per_s": nbytes / ms / 1e6,
           "hbm_fraction": nbytes / ms / 1e6 / args.hbm_peak, "beats": int(b.count.sum())}
    if not args.no_torch:
        tms, tall = _event_ms(lambda: torch_detect(x[:args.torch_records], args.fs), max(2, args.reps // 2), 1)
        tms *= args.records / min(args.records, args.torch_records)            # (scaled to the same number of records)
        mine, theirs = b.tolist(), [p.tolist() for p in torch_detect(x[:args.torch_records], args.fs)]
        leg.update(torch_ms=tms, torch_records=min(args.records, args.torch_records), torch_over_detect=tms / ms,
                   agree=float(np.mean([p == q for p, q in zip(mine, theirs)])))
    return leg


def pool_leg(args):
    fs, S = args.fs, args.streams
    secs = args.warm + args.calls + int(np.ceil(beat_latency(fs))) + 1
    x = _records(min(S, 4), args.leads, secs * fs)
    pool = BeatPool(args.leads, S, fs, device=DEV)
    sids = [pool.open() for _ in range(S)]
    ts, beats = [], 0
    for i in range(secs):
        chunks = {sid: x[s % x.shape[0], :, i * fs:(i + 1) * fs] for s, sid in enumerate(sids)}
        t0 = time.perf_counter()
        res = pool.push(chunks)
        dt = time.perf_counter() - t0
        if i >= secs - args.calls:
            ts.append(1e3 * dt)
            beats += sum(len(v) for v in res.values())
    p99 = sorted(ts)[max(0, -(-99 * len(ts) // 100) - 1)]
    med = _median(ts)
    return {"S": S, "leads": args.leads, "fs": fs, "chunk": fs, "calls": len(ts), "push_median_ms": med, "push_p99_ms": p99,
            "samples_per_s": S * fs / med * 1e3, "times_real_time": 1e3 / med, "beats": beats,
            "latency_s": beat_latency(fs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=64)
    ap.add_argument("--leads", type=int, default=2)
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--fs", type=int, default=360)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--hbm-peak", type=float, default=8000.0, help="GB/s")
    ap.add_argument("--torch-records", type=int, default=64, help="records the torch pipeline runs (its time is scaled up)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--legs", default="records,pool")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beat_bench: needs a HIP device")
    res = {"tool": "beat_bench", "geometry": beat_geometry(args.fs)}
    if "records" in args.legs:
        res["records"] = records_leg(args)
        torch.cuda.empty_cache()
    if "pool" in args.legs:
        res["pool"] = pool_leg(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
