"""Heart-rate variability on the device: what `HrvAnalyzer.analyse` and `HrvPool.push` cost.

Three legs:
  records  `HrvAnalyzer.analyse` on `--lists` beat lists of `--minutes` minutes at `--fs` Hz with the default geometry (windows of
           300 s every 60 s): the lists from `synth.make_beats_with_hrv` with V and S beats, uploaded once as a `Beats` with
           labels; ms per call (device events around `--reps` calls after `--warm`, the median) and windows per second, without
           and with the psd output.
  oracle   the numpy restatement of the definition (tests/hrv_util.py, fp64) on `--oracle-lists` of the same lists, a host clock:
           windows per second, for orientation only (one CPU thread against a GPU).
  pool     `HrvPool.push` with `--streams` streams of `--leads` leads fed `--chunk-s` seconds of synthetic ECG per stream and call
           until `--pool-s` seconds have gone in, then closed: ms per push (host clock around the call, which synchronises;
           median and p99) over all pushes after `--warm`, and the windows the pool gave per second of wall time; beside it the
           same pushes into a `BeatClassPool` alone.

Prints one JSON line.  Needs a HIP device: there is no fallback.

    python tools/hrv_bench.py [--lists 64] [--minutes 30] [--fs 360] [--reps 10] [--warm 3] [--oracle-lists 2] [--streams 64]
                              [--leads 2] [--chunk-s 10] [--pool-s 1800] [--legs records,oracle,pool]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from ecg_denoise_amd import BeatClassPool, Beats, HrvAnalyzer, HrvPool, synth  # noqa: E402
from ecg_denoise_amd.intake import pad_rows  # noqa: E402

DEV = "cuda:0"


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


def _lists(args):
    T = args.minutes * 60 * args.fs
    return T, synth.make_beats_with_hrv(args.lists, T, fs=args.fs, seed=7, p_v=0.03, p_s=0.03)


def records_leg(args):
    T, (beats, labels) = _lists(args)
    ana = HrvAnalyzer(args.fs, device=DEV)
    b = Beats(torch.from_numpy(pad_rows(beats, -1)).to(DEV), torch.tensor([len(p) for p in beats], dtype=torch.int32, device=DEV), args.fs)
    lab = torch.from_numpy(pad_rows(labels, -1)).to(DEV)
    from ecg_denoise_amd.rhythm import BeatClasses
    classes = BeatClasses(lab, None, None, b.count, b.peaks, 0.7, 0.8, args.fs)
    out = {"lists": args.lists, "T": T, "fs": args.fs, "beats": int(b.count.sum()),
           "geometry": {k: v for k, v in ana.geometry.items() if k in ("W", "H", "F", "lo_n", "hi_n", "max_m", "min_nn")}}
    for name, psd in (("analyse", False), ("analyse_psd", True)):
        ms, all_ms = _event_ms(lambda: ana.analyse(b, T, classes, psd=psd), args.reps, args.warm)
        out[name + "_ms"], out[name + "_ms_all"] = ms, all_ms
    h = ana.analyse(b, T, classes)
    out["windows"] = len(h)
    out["windows_per_s"] = len(h) / out["analyse_ms"] * 1e3
    out["mean_n_nn"] = float(h.n_nn.float().mean())
    return out


def oracle_leg(args):
    import hrv_util as U
    T, (beats, labels) = _lists(args)
    g = HrvAnalyzer(args.fs, device=DEV).geometry
    n = min(args.oracle_lists, args.lists)
    t0 = time.perf_counter()
    w = sum(len(U.oracle_record(beats[r], labels[r], T, g)) for r in range(n))
    dt = time.perf_counter() - t0
    return {"lists": n, "windows": w, "seconds": dt, "windows_per_s": w / dt}


def pool_leg(args):
    fs, S, c = args.fs, args.streams, args.chunk_s * args.fs
    T = args.pool_s * fs
    x = torch.tensor(synth.make_records_with_rhythm(min(S, 4), args.leads, T, seed=5)[0], device=DEV)
    out = {}
    for name, pool in (("push", HrvPool(args.leads, S, fs, device=DEV)), ("classes_push", BeatClassPool(args.leads, S, fs, device=DEV))):
        sids = [pool.open() for _ in range(S)]
        ts, windows, t_all = [], 0, 0.0
        for i, lo in enumerate(range(0, T, c)):
            chunks = {sid: x[s % x.shape[0], :, lo:lo + c] for s, sid in enumerate(sids)}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pool.push(chunks, close=sids if lo + c >= T else ())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if i >= args.warm:
                ts.append(1e3 * dt)
                t_all += dt
                if name == "push":
                    windows += sum(len(v) for v in res.values())
        out[name + "_median_ms"] = _median(ts)
        out[name + "_p99_ms"] = sorted(ts)[max(0, -(-99 * len(ts) // 100) - 1)]
        if name == "push":
            out["windows"], out["windows_per_s"] = windows, windows / t_all
    out.update(S=S, leads=args.leads, fs=fs, chunk=c, seconds_per_stream=args.pool_s,
               times_real_time=1e3 * args.chunk_s / out["push_median_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=64)
    ap.add_argument("--minutes", type=int, default=30)
    ap.add_argument("--fs", type=int, default=360)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--oracle-lists", type=int, default=2)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--leads", type=int, default=2, help="leads of the pool leg")
    ap.add_argument("--chunk-s", type=int, default=10)
    ap.add_argument("--pool-s", type=int, default=1800)
    ap.add_argument("--legs", default="records,oracle,pool")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hrv_bench: needs a HIP device")
    res = {"tool": "hrv_bench"}
    if "records" in args.legs:
        res["records"] = records_leg(args)
    if "oracle" in args.legs:
        res["oracle"] = oracle_leg(args)
    if "pool" in args.legs:
        res["pool"] = pool_leg(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
