"""Live streams through `LiveDenoiser`: per-push latency and throughput against offline streaming of the same signal.

RALENet("full", leads=2, L=512, max_batch=4096) at 360 Hz.  For S streams in {1, 64, 1024, 4096} and chunks of C in
{hop, 4 hop} samples, with hipGraph replay and eagerly, the object is pushed into its steady state (the lag constant, both
graphs captured), then `--pushes` pushes are timed one by one with the host clock around a device synchronise (the copy of
the chunk into the object's input buffer included; the chunks come from a device buffer).  Reported per leg: median and p99
push latency, windows/s (S C / hop windows per push over the mean push time) and the real-time factor: seconds of signal of
all S streams (S C / 360 per push) per wall-second.

In the same process `StreamingDenoiser(model, batch=4096)` denoises the S = 4096 signal offline (records of `--offline-T`
samples, one hipGraph replay per group, device events around `--reps` replays): `offline_windows_per_s` is the yardstick
for the live legs.  Prints one JSON line.

    python tools/live_bench.py [--overlap 0] [--streams 1,64,1024,4096] [--pushes 30]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ecg_denoise_amd import RALENet  # noqa: E402
from ecg_denoise_amd.infer import LiveDenoiser, StreamingDenoiser  # noqa: E402

DEV = "cuda:0"
FS = 360.0


def _signal(S, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float32) / FS
    beat = torch.exp(-((t * 1.2) % 1.0 - 0.3) ** 2 / 2e-4)
    scale = 500 + 500 * torch.rand(S, 2, 1, generator=g)
    return (beat * scale + 100 * torch.randn(S, 2, 1, generator=g) + 20 * torch.randn(S, 2, T, generator=g)).contiguous()


def _live_leg(m, sig, S, C, overlap, use_graph, pushes):
    L = m.eng.L
    hop = L - overlap
    K = sig.shape[2] // C                                # chunks in the signal buffer, used in turn
    ld = LiveDenoiser(m, streams=S, chunk=C, overlap=overlap, use_graph=use_graph)
    i = 0

    def push():
        nonlocal i
        y = ld.push(sig[:S, :, (i % K) * C:(i % K + 1) * C], copy=False)
        i += 1
        return y

    while ld.samples_in < L + 2 * C:                     # the first window, then both parities in the steady state
        push()
    torch.cuda.synchronize()
    ts = []
    for _ in range(pushes):
        t0 = time.perf_counter()
        push()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    mean = sum(ts) / len(ts)
    nw = S * (C // hop)
    return {"S": S, "C": C, "graph": use_graph, "windows_per_push": nw, "pushes": pushes,
            "median_ms": 1e3 * ts[len(ts) // 2], "p99_ms": 1e3 * ts[min(len(ts) - 1, int(0.99 * len(ts)))],
            "windows_per_s": nw / mean, "realtime_factor": S * C / FS / mean}


def _offline(m, sig, overlap, reps):
    sd = StreamingDenoiser(m, batch=4096, overlap=overlap, use_graph=True)
    nw = sig.shape[0] * sd.windows_per_record(sig.shape[2])
    sd.denoise(sig, copy=False)
    sd.denoise(sig, copy=False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        sd.denoise(sig, copy=False)
    e1.record()
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1) / 1e3 / reps
    return {"records": sig.shape[0], "T": sig.shape[2], "windows": nw, "s_per_group": t, "windows_per_s": nw / t,
            "realtime_factor": sig.shape[0] * sig.shape[2] / FS / t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=0)
    ap.add_argument("--streams", default="1,64,1024,4096")
    ap.add_argument("--cmul", default="1,4", help="chunk lengths in multiples of hop")
    ap.add_argument("--modes", default="graph,eager")
    ap.add_argument("--pushes", type=int, default=30)
    ap.add_argument("--offline-T", type=int, default=8 * 512)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("live_bench: needs a HIP device")
    L, ov = args.L, args.overlap
    hop = L - ov
    streams = [int(v) for v in args.streams.split(",")]
    cmuls = [int(v) for v in args.cmul.split(",")]
    m = RALENet("full", leads=2, L=L, max_batch=4096, train=False, device=DEV, seed=1).eval()
    Smax = max(streams)
    T = max(args.offline_T, 4 * max(cmuls) * hop)
    sig = _signal(Smax, T).to(DEV)
    res = {"tool": "live_bench", "model": "full", "leads": 2, "L": L, "overlap": ov, "hop": hop, "fs": FS, "legs": []}
    res["offline"] = _offline(m, sig, ov, args.reps)
    for S in streams:
        for cm in cmuls:
            for mode in args.modes.split(","):
                res["legs"].append(_live_leg(m, sig, S, cm * hop, ov, mode == "graph", args.pushes))
                torch.cuda.empty_cache()
    off = res["offline"]["windows_per_s"]
    for leg in res["legs"]:
        leg["vs_offline"] = leg["windows_per_s"] / off
    print(json.dumps(res))


if __name__ == "__main__":
    main()
