"""Independent live streams through `LivePool`: per-call latency and throughput for three traffic mixes.

RALENet("full", leads=2, L=512, max_batch=4096), overlap 0 (hop 512), S streams in {64, 1024, 4096}:

  lockstep  every stream gets C = hop samples per call.  Two eager `LiveDenoiser` objects and the pool run on the same chunks,
            alternating call by call in one process: `pool_over_live` is the pool's median over the first LiveDenoiser's, and
            `live_over_live` the second LiveDenoiser's over the first's (the spread of the yardstick against itself).
  packets   every stream gets 360 samples per call (one second at 360 Hz); the streams' start phases are spread over the hop,
            so about 360 / 512 of them complete a window in a given call.
  churn     as packets, and a seeded fraction of the streams (`--churn`, of those that have a window's worth of samples) is
            closed with its chunk in a call and reopened before the next one.

A call is timed with the host clock around a device synchronise, `--calls` calls after `--warm` warm-up calls of the same mix
(the chunk dictionary is prepared before the clock starts; the chunks are contiguous device tensors).  Reported per leg: median,
p99 and maximum ms per call (`--calls` 100 by default, at least 30), windows per call (mean) and windows/s; with `--split` the
lockstep legs also report the host milliseconds per call of the steps of the pool's `push` around its launches (`_host_split`).  Prints one JSON line.  Needs a HIP device: there is no fallback.

    python tools/pool_bench.py [--streams 64,1024,4096] [--mixes lockstep,packets,churn] [--calls 100] [--warm 8] [--split]
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

from ecg_denoise_amd import LiveDenoiser, LivePool, RALENet  # noqa: E402

DEV = "cuda:0"
FS, L, PACKET = 360.0, 512, 360


def _blocks(S, C, K, seed=0):
    """K chunks (S, 2, C) of an ECG-like signal, each contiguous on the device"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(K * C, dtype=torch.float32) / FS
    beat = torch.exp(-((t * 1.2) % 1.0 - 0.3) ** 2 / 2e-4)
    sig = beat * (500 + 500 * torch.rand(S, 2, 1, generator=g)) + 20 * torch.randn(S, 2, K * C, generator=g)
    return [sig[:, :, i * C:(i + 1) * C].contiguous().to(DEV) for i in range(K)]


def _stats(ts, windows):
    """p99: the smallest time that 99 % of the calls stay at or below (the second largest of 100 calls); max beside it"""
    ts = sorted(ts)
    return {"calls": len(ts), "median_ms": 1e3 * ts[len(ts) // 2], "p99_ms": 1e3 * ts[max(0, -(-99 * len(ts) // 100) - 1)],
            "max_ms": 1e3 * ts[-1], "windows_per_call": windows / len(ts), "windows_per_s": windows / sum(ts)}


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _host_split(pool, chunks, reps):
    """host ms per call of the steps of `LivePool.push` around its launches, each repeated on its own outside a push: the plan
    (argument checks and table, `PoolState.plan`; nothing is committed), the packing of the chunks (one `torch.cat`, device
    synchronised) and the result dictionary of per-stream views"""
    t = {"plan": 0.0, "pack": 0.0, "result": 0.0}
    leads = pool.leads
    for _ in range(reps):
        t0 = time.perf_counter()
        sids, tab, _ = pool.state.plan({sid: tuple(x.shape) for sid, x in chunks.items()})
        t1 = time.perf_counter()
        xp = torch.cat([x.reshape(-1) for x in chunks.values()])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        parts = xp[:int(tab["c"].sum()) * leads].split([int(v) * leads for v in tab["c"]])
        res = {sid: p.view(leads, -1) for sid, p in zip(sids, parts)}
        t3 = time.perf_counter()
        t["plan"] += t1 - t0
        t["pack"] += t2 - t1
        t["result"] += t3 - t2
    return {k: 1e3 * v / reps for k, v in t.items()}


def _lockstep(m, S, calls, warm, split):
    blocks = _blocks(S, L, 4)
    live = [LiveDenoiser(m, streams=S, chunk=L, overlap=0, use_graph=False) for _ in range(2)]
    pool = LivePool(m, capacity=S, overlap=0)
    sids = [pool.open() for _ in range(S)]
    ts = {"live_a": [], "live_b": [], "pool": []}
    for i in range(warm + calls):
        x = blocks[i % 4]
        chunks = {sid: x[s] for s, sid in enumerate(sids)}
        for name, fn in (("live_a", lambda: live[0].push(x)), ("live_b", lambda: live[1].push(x)),
                         ("pool", lambda: pool.push(chunks))):
            dt = _timed(fn)
            if i >= warm:
                ts[name].append(dt)
    res = {"mix": "lockstep", "S": S, "C": L}
    res.update({name: _stats(t, S * calls) for name, t in ts.items()})
    res["pool_over_live"] = res["pool"]["median_ms"] / res["live_a"]["median_ms"]
    res["live_over_live"] = res["live_b"]["median_ms"] / res["live_a"]["median_ms"]
    if split:
        res["pool_host_ms"] = _host_split(pool, chunks, calls)
    return res


def _packets(m, S, calls, warm, churn, seed=1):
    blocks = _blocks(S, PACKET, 4)
    rng = np.random.default_rng(seed)
    pool = LivePool(m, capacity=S, overlap=0)
    sids = [pool.open() for _ in range(S)]
    phase = blocks[0][:, :, :]                       # start phases spread over the hop: 1 + (37 s mod hop) samples first
    pool.push({sid: phase[s, :, :1 + (37 * s) % min(L, PACKET)].contiguous() for s, sid in enumerate(sids)})
    ts, w0, closed = [], 0, 0
    for i in range(warm + calls):
        x = blocks[i % 4]
        chunks = {sid: x[s] for s, sid in enumerate(sids)}
        close = []
        if churn:
            ready = [s for s, sid in enumerate(sids) if pool.samples_in(sid) + PACKET >= L]
            close = [sids[s] for s in rng.choice(ready, size=min(len(ready), max(1, int(churn * S))), replace=False)] if ready else []
        if i == warm:
            w0 = pool.windows_run
        dt = _timed(lambda: pool.push(chunks, close=close))
        if i >= warm:
            ts.append(dt)
            closed += len(close)
        back = {sid: pool.open() for sid in close}    # the freed slots, taken again before the next call
        sids = [back.get(sid, sid) for sid in sids]
    res = {"mix": "churn" if churn else "packets", "S": S, "C": PACKET}
    res.update(_stats(ts, pool.windows_run - w0))
    if churn:
        res["closed_per_call"] = closed / calls
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="64,1024,4096")
    ap.add_argument("--mixes", default="lockstep,packets,churn")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--split", action="store_true",
                    help="lockstep: also the host time of the steps of push around its launches (plan, pack, result)")
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--churn", type=float, default=0.02, help="fraction of the streams closed and reopened per call")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_bench: needs a HIP device")
    if args.calls < 30:
        raise SystemExit("pool_bench: at least 30 timed calls")
    m = RALENet("full", leads=2, L=L, max_batch=4096, train=False, device=DEV, seed=1).eval()
    res = {"tool": "pool_bench", "model": "full", "leads": 2, "L": L, "overlap": 0, "calls": args.calls, "warm": args.warm,
           "churn": args.churn, "legs": []}
    for S in (int(v) for v in args.streams.split(",")):
        for mix in args.mixes.split(","):
            if mix == "lockstep":
                res["legs"].append(_lockstep(m, S, args.calls, args.warm, args.split))
            else:
                res["legs"].append(_packets(m, S, args.calls, args.warm, args.churn if mix == "churn" else 0.0))
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
