"""Sample-rate conversion around the streaming denoisers: what the two conversions cost, per call and end to end.

Two workloads of 30-minute records (`--minutes`):
  newrale  R 12-lead records at 500 Hz through NewRALE(RALENet("full", leads=2, L=512, max_batch=4096))
  full     R 2-lead records at 250 Hz through RALENet("full", leads=2, L=512, max_batch=4096)

Per workload:
  convert   `Resampler.convert` to 360 Hz and back, each on its own: ms per call (device events around `--reps` calls after
            `--warm`, the median) and GB/s against the 4 (T + T_out) leads R bytes the conversion has to move.
  stream    `RateStreamingDenoiser.denoise` at the record's rate against `StreamingDenoiser.denoise` on records of the same
            duration at 360 Hz, alternating call by call in one process; `rate_over_native` is the ratio of the medians and
            `convert_share` the two conversions' ms over the RateStreamingDenoiser's.
  pool      `RateLivePool.push` against `LivePool.push` (`NewRALELivePool` for the 12-lead model): `--streams` streams, one
            second of samples per stream and call (fs at the record's rate, 360 at the model's), median / p99 ms per push
            (host clock around a device synchronise), alternating call by call.

Prints one JSON line.  Needs a HIP device: there is no fallback.

    python tools/rate_bench.py [--records 4] [--minutes 30] [--streams 64] [--reps 20] [--warm 3] [--calls 60]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ecg_denoise_amd import (LivePool, NewRALE, NewRALELivePool, RALENet, RateLivePool, RateStreamingDenoiser,  # noqa: E402
                             Resampler, rate_latency)
from ecg_denoise_amd.infer import StreamingDenoiser  # noqa: E402

DEV = "cuda:0"
FS_MODEL, L = 360, 512


def _records(R, leads, T, fs, seed=0):
    """ADC-like ECG records at `fs`: a beat train on a baseline of 1024, per-record and per-lead amplitude, noise"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float32) / fs
    beat = torch.exp(-((t * 1.2) % 1.0 - 0.3) ** 2 / 2e-4)
    return (1024 + beat * (100 + 300 * torch.rand(R, leads, 1, generator=g)) + 20 * torch.randn(R, leads, T, generator=g)).to(DEV)


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def _event_ms(fn, reps, warm):
    """median ms of one call, device events around each of `reps` calls"""
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
    return _median(ts)


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _convert(x, fs_in, fs_out, reps, warm):
    rs = Resampler(fs_in, fs_out, DEV)
    R, leads, T = x.shape
    ms = _event_ms(lambda: rs.convert(x), reps, warm)
    T_out = rs.length(T)
    nbytes = 4 * (T + T_out) * leads * R
    return {"fs_in": fs_in, "fs_out": fs_out, "up": rs.up, "down": rs.down, "R": R, "leads": leads, "T": T, "T_out": T_out,
            "ms": ms, "bytes": nbytes, "GB_per_s": nbytes / ms / 1e6}, rs.convert(x)


def _stream(model, x, x360, fs, reps, warm, conv_ms):
    rate, native = RateStreamingDenoiser(model, fs), StreamingDenoiser(model)
    ts = {"rate": [], "native": []}
    for i in range(warm + reps):
        for name, fn in (("native", lambda: native.denoise(x360, copy=False)), ("rate", lambda: rate.denoise(x))):
            dt = _timed(fn)
            if i >= warm:
                ts[name].append(dt)
    r, n = 1e3 * _median(ts["rate"]), 1e3 * _median(ts["native"])
    return {"rate_ms": r, "native_ms": n, "rate_over_native": r / n, "convert_ms": conv_ms, "convert_share": conv_ms / r,
            "convert_over_native": conv_ms / n}


def _pool(model, leads, x, x360, fs, S, calls, warm):
    adapter = isinstance(model, NewRALE)
    rate, native = RateLivePool(model, fs, capacity=S), (NewRALELivePool if adapter else LivePool)(model, capacity=S)
    sr, sn = [rate.open() for _ in range(S)], [native.open() for _ in range(S)]
    R = x.shape[0]
    ts = {"rate": [], "native": []}
    for i in range(warm + calls):
        cr = {sid: x[s % R, :, i * fs:(i + 1) * fs] for s, sid in enumerate(sr)}
        cn = {sid: x360[s % R, :, i * FS_MODEL:(i + 1) * FS_MODEL] for s, sid in enumerate(sn)}
        for name, fn in (("native", lambda: native.push(cn)), ("rate", lambda: rate.push(cr))):
            dt = _timed(fn)
            if i >= warm:
                ts[name].append(dt)
    p99 = lambda t: sorted(t)[max(0, -(-99 * len(t) // 100) - 1)]
    r, n = 1e3 * _median(ts["rate"]), 1e3 * _median(ts["native"])
    return {"S": S, "calls": calls, "rate_median_ms": r, "rate_p99_ms": 1e3 * p99(ts["rate"]), "native_median_ms": n,
            "native_p99_ms": 1e3 * p99(ts["native"]), "rate_over_native": r / n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=4)
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--workloads", default="newrale,full")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rate_bench: needs a HIP device")
    secs = int(args.minutes * 60)
    if secs < args.calls + args.warm + 2:
        raise SystemExit("rate_bench: the records must be longer than the pool leg's calls (one second each)")
    res = {"tool": "rate_bench", "L": L, "minutes": args.minutes, "records": args.records, "reps": args.reps, "warm": args.warm,
           "legs": []}
    for name in args.workloads.split(","):
        inner = RALENet("full", leads=2, L=L, max_batch=4096, train=False, device=DEV, seed=1).eval()
        model, leads, fs = (NewRALE(inner, seed=2).eval(), 12, 500) if name == "newrale" else (inner, 2, 250)
        x = _records(args.records, leads, secs * fs, fs)
        x360 = _records(args.records, leads, secs * FS_MODEL, FS_MODEL)
        leg = {"workload": name, "leads": leads, "fs": fs, "latency_samples_in": rate_latency(fs, FS_MODEL),
               "latency_samples_back": rate_latency(FS_MODEL, fs)}
        leg["to_model"], xm = _convert(x, fs, FS_MODEL, args.reps, args.warm)
        leg["back"], _ = _convert(xm, FS_MODEL, fs, args.reps, args.warm)
        del xm
        leg["stream"] = _stream(model, x, x360, fs, max(5, args.reps // 2), args.warm, leg["to_model"]["ms"] + leg["back"]["ms"])
        leg["pool"] = _pool(model, leads, x, x360, fs, args.streams, args.calls, args.warm)
        res["legs"].append(leg)
        del x, x360, model, inner
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
