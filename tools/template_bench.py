"""Median beats on the device: what `MedianBeat.average` costs, beside a torch restatement on the same device.

`--shapes` (default 64x2x648000@360 and 16x12x900000@500: records x leads x samples @ rate, 30 minutes each) are synthetic rhythm
records (at most four distinct ones, repeated; the 500 Hz records are the same samples read at 500 Hz) with the generator's
beats and labels, uploaded once; windows of `--win` seconds every `--hop` (10, 10).  `average` is timed with device events
around `--reps` calls after `--warm` (the median) and reported as ms per call, used beats/s and two byte rates: `record_GBps`,
the record's own bytes over the time - every sample should come from HBM about once, so this is the rate to hold against the
memory's - and `moved_GBps`, the bytes the kernel asks for (every used beat's Wn samples of every lead, the lists, the
templates written) over the time.

The restatement gathers the member windows into (windows, K, leads, Wn) with K the largest count, padded with +inf, sorts along
K with `torch.sort` and takes the middle value or the mean of the two middle values; its index tensors are built outside the
timed region, it runs in chunks of `--chunk` records, and its result is compared with the kernel's for equality.

Prints one JSON line.  Needs a HIP device: there is no fallback.

    python tools/template_bench.py [--shapes 64x2x648000@360,16x12x900000@500] [--win 10] [--hop 10] [--reps 10] [--warm 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ecg_denoise_amd import Beats, MedianBeat, synth  # noqa: E402
from ecg_denoise_amd.intake import pad_rows  # noqa: E402

DEV = "cuda:0"


def _records(R, leads, T, distinct=4):
    """-> (records on the device, beat lists, label lists), at most `distinct` different records"""
    x, beats, labels = synth.make_records_with_rhythm(min(R, distinct), leads, T, seed=5)
    n = x.shape[0]
    rec = torch.tensor(x, device=DEV).repeat(-(-R // n), 1, 1)[:R].contiguous()
    return rec, [beats[r % n] for r in range(R)], [labels[r % n] for r in range(R)]


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


def _member_table(beats, labels, T, g, win):
    """-> per record and window the start p - Wpre of every used beat: (R, nw, K) int64 padded with 0, and the counts (R, nw)"""
    rows = []
    for pos, lab in zip(beats, labels):
        pos, lab = np.asarray(pos, dtype=np.int64), np.asarray(lab)
        ok = (lab == 0) & (pos - g["Wpre"] >= 0) & (pos + g["Wpost"] <= T - 1)
        rows.append([(pos[ok & (pos >= w0) & (pos < w1)] - g["Wpre"])[:g["KMAX"]] for w0, w1 in win])
    K = max(1, max(len(m) for row in rows for m in row))
    start = np.stack([pad_rows(row, 0, np.int64, (len(win), K)) for row in rows])
    return torch.from_numpy(start).to(DEV), torch.tensor([[len(m) for m in row] for row in rows], device=DEV)


def _restatement(x, start, n, Wn, chunk):
    """gather, `torch.sort`, take the middle -> (R, nw, leads, Wn)"""
    out = []
    k = torch.arange(Wn, device=x.device)
    inf = torch.tensor(float("inf"), device=x.device)
    for a in range(0, x.shape[0], chunk):
        xs, st, cnt = x[a:a + chunk], start[a:a + chunk], n[a:a + chunk]
        r = torch.arange(xs.shape[0], device=x.device)[:, None, None, None, None]
        l = torch.arange(xs.shape[1], device=x.device)[None, None, None, :, None]
        v = xs[r, l, st[:, :, :, None, None] + k]                                     # (R, nw, K, leads, Wn)
        valid = torch.arange(st.shape[2], device=x.device)[None, None, :] < cnt[:, :, None]
        v = torch.sort(torch.where(valid[..., None, None], v, inf), dim=2).values
        lo = ((cnt - 1).clamp(min=0) // 2)[:, :, None, None, None].expand(-1, -1, 1, v.shape[3], Wn)
        hi = (cnt // 2).clamp(max=st.shape[2] - 1)[:, :, None, None, None].expand(-1, -1, 1, v.shape[3], Wn)
        vlo, vhi = v.gather(2, lo)[:, :, 0], v.gather(2, hi)[:, :, 0]
        odd = (cnt % 2 == 1)[:, :, None, None]
        out.append(torch.where((cnt > 0)[:, :, None, None], torch.where(odd, vlo, (vlo + vhi) * 0.5), torch.zeros_like(vlo)))
    return torch.cat(out)


def leg(args, R, leads, T, fs):
    x, beats, labels = _records(R, leads, T)
    mb = MedianBeat(fs, win_s=args.win, hop_s=args.hop, device=DEV)
    g = mb.geometry
    peaks = torch.from_numpy(pad_rows(beats, -1)).to(DEV)
    lab = torch.from_numpy(pad_rows(labels, -1, shape=tuple(peaks.shape))).to(DEV)
    b = Beats(peaks, torch.tensor([len(p) for p in beats], dtype=torch.int32, device=DEV), fs)
    ms, all_ms = _event_ms(lambda: mb.average(x, b, lab), args.reps, args.warm)
    t = mb.average(x, b, lab)
    start, n = _member_table(beats, labels, T, g, t.index)
    tms, all_tms = _event_ms(lambda: _restatement(x, start, n, g["Wn"], args.chunk), max(2, args.reps // 2), 1)
    ref = _restatement(x, start, n, g["Wn"], args.chunk)
    used = int(t.used.sum())
    record_bytes = 4 * R * leads * T
    moved = 4 * (used * leads * g["Wn"] + t.template.numel() + 2 * int(b.count.sum()) + 3 * t.used.numel())
    return {"R": R, "leads": leads, "T": T, "fs": fs, "Wn": g["Wn"], "W": g["W"], "H": g["H"], "windows": int(t.used.numel()),
            "beats": int(b.count.sum()), "used_beats": used, "cap": int(peaks.shape[1]), "largest_count": int(t.used.max()),
            "average_ms": ms, "average_ms_all": all_ms, "beats_per_s": used / ms * 1e3, "record_bytes": record_bytes,
            "record_GBps": record_bytes / ms / 1e6, "moved_bytes": moved, "moved_GBps": moved / ms / 1e6,
            "torch_ms": tms, "torch_ms_all": all_tms, "torch_over_kernel": tms / ms,
            "equals_torch": bool(torch.equal(n.to(torch.int32), t.used) and (ref == t.template).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x2x648000@360,16x12x900000@500")
    ap.add_argument("--win", type=int, default=10)
    ap.add_argument("--hop", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=8, help="records per pass of the torch restatement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("template_bench: needs a HIP device")
    res = {"tool": "template_bench", "legs": []}
    for shape in [s for s in args.shapes.split(",") if s]:
        dims, fs = shape.split("@")
        R, leads, T = (int(v) for v in dims.split("x"))
        res["legs"].append(leg(args, R, leads, T, int(fs)))
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
