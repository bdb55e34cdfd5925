"""Throughput of 12-lead record streaming through `NewRALE` (BASELINE config 5 shapes with the 12-lead model of config 4).

R records of (12, T) samples (T = 650 000: 30 minutes at 360 Hz) go through
NewRALE(RALENet("full", leads=2, L=1024, max_batch=4096)) in batches of 4096 windows, at overlap 0 and 128, as hipGraphs:

  fused    StreamingDenoiser(NewRALE): ral_newrale_stream_front -> ral_forward -> ral_newrale_stream_back per batch
  unfused  the same pipeline from the entry points that existed before: ral_stream_windows(leads=12) -> 2 x ral_conv13_forward
           -> ral_forward -> 2 x ral_conv13_forward per batch, one ral_stream_stitch(leads=12) per group

Both are timed with device events around `--reps` graph replays after `--warmup` replays.  Prints one JSON line:
windows/s and record-seconds/s of both paths per overlap, the fused/unfused ratio and the rel-L2 between the two outputs.

`--profile` also runs the fused path in a child process under `rocprofv3 --kernel-trace --stats` (output under
`--out`, default build/newrale_stream_prof, kept out of git) and adds `profile`: the kernel time of the run and the share of it spent
in k_newrale_front, k_newrale_back and in everything else (the inner model), from rocprofv3's kernel_stats.csv or, with
its rocpd output, the `kernels` view of its SQLite database.  That share is of the summed kernel durations, not of wall
time; the child also replays warm-up graphs, which only adds calls to the same kernels in the same proportions.

Measured on one MI355X (R = 8, T = 650 000, batch 4096): overlap 0: 183 600 windows/s fused against 175 000
unfused (x 1.049), overlap 128: 183 600 against 178 700 (x 1.027), outputs identical (rel-L2 0.0).  Kernel-time share
at overlap 0: k_newrale_front 0.85 % (223 us per 4096-or-984-window call), k_newrale_back 0.31 %, the inner model 98.8 %.

    python tools/newrale_stream_bench.py [--records 8] [--T 650000] [--reps 5] [--profile]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ecg_denoise_amd import NewRALE, RALENet, _lib  # noqa: E402
from ecg_denoise_amd.infer import StreamingDenoiser  # noqa: E402
from ecg_denoise_amd.model import _ptr, _stream  # noqa: E402

DEV = "cuda:0"
FS = 360.0


def _records(R, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float32) / FS
    beat = torch.exp(-((t * 1.2) % 1.0 - 0.3) ** 2 / 2e-4)
    scale = 500 + 500 * torch.rand(R, 12, 1, generator=g)
    return (beat * scale + 100 * torch.randn(R, 12, 1, generator=g) + 20 * torch.randn(R, 12, T, generator=g)).contiguous()


class Unfused:
    """the record pipeline from the pre-existing entry points, captured into one hipGraph per group"""

    def __init__(self, m, R, T, L, hop, batch):
        self.m, self.R, self.T, self.L, self.hop, self.batch = m, R, T, L, hop, batch
        n = (T - L) // hop + 1 + (1 if (T - L) % hop else 0)
        self.nw_all = R * n
        nb = min(batch, self.nw_all)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
        self.rec, self.out, self.stats = z(R, 12, T), z(R, 12, T), z(self.nw_all * 24)
        self.win, self.a1, self.a2, self.r, self.a3 = z(nb, 12, L), z(nb, 6, L), z(nb, 2, L), z(nb, 2, L), z(nb, 6, L)
        self.y = z(self.nw_all, 12, L)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            self._run()
        torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._run()

    def _conv(self, name, x, y, nw, cin, cout, lrelu):
        m = self.m
        w, b = m._view(m.params, name + ".weight"), m._view(m.params, name + ".bias")
        _lib.check(_lib.lib().ral_conv13_forward(_ptr(x), _ptr(w), _ptr(b), _ptr(y), nw, cin, cout, self.L, int(lrelu), _stream()))

    def _run(self):
        lib, R, T, L, hop = _lib.lib(), self.R, self.T, self.L, self.hop
        for w0 in range(0, self.nw_all, self.batch):
            nw = min(self.batch, self.nw_all - w0)
            _lib.check(lib.ral_stream_windows(_ptr(self.rec), R, T, 12, L, hop, w0, nw, _ptr(self.win), _ptr(self.stats), _stream()))
            self._conv("conv1", self.win, self.a1, nw, 12, 6, True)
            self._conv("conv2", self.a1, self.a2, nw, 6, 2, True)
            _lib.check(lib.ral_forward(self.m.rale.eng.h, _ptr(self.a2), _ptr(self.r), nw, 0, _stream()))
            self._conv("conv3", self.r, self.a3, nw, 2, 6, True)
            self._conv("conv4", self.a3, self.y[w0:], nw, 6, 12, False)
        _lib.check(lib.ral_stream_stitch(_ptr(self.y), _ptr(self.stats), R, T, 12, L, hop, _ptr(self.out), _stream()))

    def denoise(self, rec):
        self.rec.copy_(rec, non_blocking=True)
        self.graph.replay()
        return self.out


def _time(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def _kernel_totals(out):
    """{kernel name: summed duration in ns} from what rocprofv3 wrote under `out`: kernel_stats.csv (csv output) or the
    `kernels` view of its SQLite database (rocpd output, the default of recent versions)"""
    tot = {}
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if files:
        for row in csv.DictReader(open(max(files, key=os.path.getmtime))):
            tot[row["Name"]] = tot.get(row["Name"], 0.0) + float(row["TotalDurationNs"])
        return tot
    dbs = glob.glob(os.path.join(out, "**", "*results.db"), recursive=True)
    if dbs:
        import sqlite3
        con = sqlite3.connect(max(dbs, key=os.path.getmtime))
        for name, ns in con.execute("SELECT name, SUM(duration) FROM kernels GROUP BY name"):
            tot[name] = float(ns)
        con.close()
    return tot


def _shares(tot):
    part = {"k_newrale_front": 0.0, "k_newrale_back": 0.0, "other": 0.0}
    for name, ns in tot.items():
        part[next((k for k in ("k_newrale_front", "k_newrale_back") if k in name), "other")] += ns
    all_ns = sum(part.values())
    return {"kernel_ms": all_ns / 1e6, "share": {k: v / all_ns for k, v in part.items()},
            "fused_share": (part["k_newrale_front"] + part["k_newrale_back"]) / all_ns}


def _profile(args):
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    ov = int(args.overlaps.split(",")[0])
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "nrs", "--", sys.executable, os.path.abspath(__file__),
           "--fused-only", "--records", str(args.records), "--T", str(args.T), "--reps", "2", "--warmup", "1",
           "--overlaps", str(ov)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.profile_timeout)
    if r.returncode != 0:
        return {"error": f"rocprofv3 exited {r.returncode}", "tail": r.stdout[-800:]}
    tot = _kernel_totals(out)
    if not tot:
        return {"error": "no kernel statistics found", "tail": r.stdout[-800:]}
    return dict(overlap=ov, **_shares(tot))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=8)
    ap.add_argument("--T", type=int, default=650000)
    ap.add_argument("--L", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--overlaps", default="0,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fused-only", action="store_true", help="time the fused path only (the run profiled by --profile)")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "newrale_stream_prof"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("newrale_stream_bench: needs a HIP device")
    R, T, L = args.records, args.T, args.L
    m = NewRALE(RALENet("full", leads=2, L=L, max_batch=args.batch, train=False, device=DEV, seed=1), seed=2).eval()
    rec = _records(R, T).to(DEV)
    res = {"tool": "newrale_stream_bench", "records": R, "T": T, "L": L, "batch": args.batch, "graph": True, "legs": []}
    for ov in [int(v) for v in args.overlaps.split(",")]:
        sd = StreamingDenoiser(m, batch=args.batch, overlap=ov, use_graph=True)
        nw = R * sd.windows_per_record(T)
        leg = {"overlap": ov, "windows": nw}
        t0 = time.time()
        sd.denoise(rec, copy=False)
        leg["fused_plan_s"] = time.time() - t0
        tf = _time(lambda: sd.denoise(rec, copy=False), args.warmup, args.reps)
        leg["fused"] = {"s_per_group": tf, "windows_per_s": nw / tf, "record_s_per_s": R * T / FS / tf}
        if not args.fused_only:
            un = Unfused(m, R, T, L, L - ov, args.batch)
            tu = _time(lambda: un.denoise(rec), args.warmup, args.reps)
            leg["unfused"] = {"s_per_group": tu, "windows_per_s": nw / tu, "record_s_per_s": R * T / FS / tu}
            leg["fused_over_unfused"] = tu / tf
            a, b = sd.denoise(rec).double(), un.denoise(rec).double()
            leg["rel_l2_fused_vs_unfused"] = float((a - b).norm() / b.norm())
            del un
        res["legs"].append(leg)
        del sd
        torch.cuda.empty_cache()
    if args.profile:
        res["profile"] = _profile(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
