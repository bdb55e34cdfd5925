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

With `--model newrale` the streams have 12 leads and run through `NewRALELiveDenoiser` around NewRALE(RALENet("full",
L = 1024)); the offline yardstick is `StreamingDenoiser(NewRALE)`.  One more leg, "unfused", times a push composed of the seven
unfused launches (ral_live_windows(leads = 12), conv1, conv2, ral_forward, conv3, conv4, ral_live_emit(leads = 12); eager) at
S = 4096, C = hop, interleaved push by push with the fused eager push on the same chunks.

    python tools/live_bench.py [--model full|newrale] [--overlap 0] [--streams 1,64,1024,4096] [--pushes 30]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ecg_denoise_amd import NewRALE, RALENet, _lib  # noqa: E402
from ecg_denoise_amd.infer import LiveDenoiser, NewRALELiveDenoiser, StreamingDenoiser, live_frontier  # noqa: E402
from ecg_denoise_amd.model import _ptr, _stream  # noqa: E402

DEV = "cuda:0"
FS = 360.0


def _signal(S, T, leads=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float32) / FS
    beat = torch.exp(-((t * 1.2) % 1.0 - 0.3) ** 2 / 2e-4)
    scale = 500 + 500 * torch.rand(S, leads, 1, generator=g)
    return (beat * scale + 100 * torch.randn(S, leads, 1, generator=g) + 20 * torch.randn(S, leads, T, generator=g)).contiguous()


def _live_object(m, S, C, overlap, use_graph):
    cls = NewRALELiveDenoiser if isinstance(m, NewRALE) else LiveDenoiser
    return cls(m, streams=S, chunk=C, overlap=overlap, use_graph=use_graph)


def _live_leg(m, sig, S, C, overlap, use_graph, pushes):
    L = m.L if isinstance(m, NewRALE) else m.eng.L
    hop = L - overlap
    K = sig.shape[2] // C                                # chunks in the signal buffer, used in turn
    ld = _live_object(m, S, C, overlap, use_graph)
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


class _UnfusedPush:
    """a 12-lead live push from the existing entry points, eagerly: ral_live_windows(leads = 12) -> conv1 -> conv2 ->
    ral_forward -> conv3 -> conv4 -> ral_live_emit(leads = 12), in batches of max_batch windows, two history buffers"""

    def __init__(self, m, S, C, overlap):
        e = m.rale.eng
        self.m, self.e, self.S, self.C, self.L, self.hop = m, e, S, C, e.L, e.L - overlap
        nw = C // self.hop
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=DEV)
        self.hist = [z(S, 12, self.L), z(S, 12, self.L)]
        self.x = z(S, 12, C)
        nb = min(e.max_batch, S * nw)
        self.win, self.y12 = z(nb, 12, self.L), z(nb, 12, self.L)
        self.a6, self.a2, self.r = z(nb, 6, self.L), z(nb, 2, self.L), z(nb, 2, self.L)
        self.stats, self.out = z(S * nw * 24), z(S, 12, C)
        self.last_y, self.last_stats = z(S, 12, self.L), z(S * 24)
        self.n, self.parity = 0, 0

    def _conv(self, name, x, y, B):
        m = self.m
        _lib.check(_lib.lib().ral_conv13_forward(_ptr(x), _ptr(m._view(m.params, name + ".weight")),
                                                 _ptr(m._view(m.params, name + ".bias")), _ptr(y), B, x.shape[1], y.shape[1],
                                                 self.L, int(name != "conv4"), _stream()))

    def push(self, x):
        lib, S, L, hop = _lib.lib(), self.S, self.L, self.hop
        n0, n1 = self.n, self.n + self.C
        nreg = lambda n: (n - L) // hop + 1 if n >= L else 0
        k0, nw = nreg(n0), nreg(n1) - nreg(n0)
        lo = live_frontier(n0, L, hop)
        m = live_frontier(n1, L, hop) - lo
        self.x.copy_(x, non_blocking=True)
        h_in, h_out = self.hist[self.parity], self.hist[1 - self.parity]
        batch = self.win.shape[0]
        for w0 in range(0, max(S * nw, 1), batch):
            nb = min(batch, S * nw - w0)
            _lib.check(lib.ral_live_windows(_ptr(h_in), _ptr(self.x), _ptr(h_out if w0 == 0 else None), S, 12, L, hop, self.C,
                                            n0 - L, k0, nw, -1, w0, nb, _ptr(self.win), _ptr(self.stats), _stream()))
            if nb == 0:
                break
            self._conv("conv1", self.win, self.a6, nb)
            self._conv("conv2", self.a6, self.a2, nb)
            _lib.check(lib.ral_forward(self.e.h, _ptr(self.a2), _ptr(self.r), nb, 0, _stream()))
            self._conv("conv3", self.r, self.a6, nb)
            self._conv("conv4", self.a6, self.y12, nb)
            _lib.check(lib.ral_live_emit(_ptr(self.y12), _ptr(self.stats), S, 12, L, hop, k0, nw, -1, w0, nb, lo, m,
                                         _ptr(self.out), _ptr(self.last_y), _ptr(self.last_stats), _stream()))
        self.n, self.parity = n1, 1 - self.parity
        return self.out


def _unfused_leg(m, sig, S, C, overlap, pushes):
    """the unfused push and the fused eager push, alternated on the same chunks; both into their steady state first"""
    K = sig.shape[2] // C
    fused, unfused = _live_object(m, S, C, overlap, False), _UnfusedPush(m, S, C, overlap)
    i = 0
    while fused.samples_in < m.L + 2 * C:
        fused.push(sig[:S, :, (i % K) * C:(i % K + 1) * C], copy=False)
        unfused.push(sig[:S, :, (i % K) * C:(i % K + 1) * C])
        i += 1
    torch.cuda.synchronize()
    ts = {"fused": [], "unfused": []}
    same = True
    for _ in range(pushes):
        ch = sig[:S, :, (i % K) * C:(i % K + 1) * C]
        for name, fn in (("fused", lambda: fused.push(ch, copy=False)), ("unfused", lambda: unfused.push(ch))):
            t0 = time.perf_counter()
            y = fn()
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t0)
            if name == "fused":
                yf = y.clone()
            else:
                same = same and torch.equal(yf, y)
        i += 1
    nw = S * (C // (m.L - overlap))
    res = {"S": S, "C": C, "windows_per_push": nw, "pushes": pushes, "outputs_equal": bool(same)}
    for name, t in ts.items():
        t.sort()
        res[name] = {"median_ms": 1e3 * t[len(t) // 2], "p99_ms": 1e3 * t[min(len(t) - 1, int(0.99 * len(t)))],
                     "windows_per_s": nw * len(t) / sum(t)}
    res["fused_over_unfused"] = res["fused"]["windows_per_s"] / res["unfused"]["windows_per_s"]
    return res


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
    ap.add_argument("--model", choices=("full", "newrale"), default="full",
                    help="full: RALENet, 2 leads; newrale: NewRALE, 12 leads (+ the unfused leg)")
    ap.add_argument("--L", type=int, default=None, help="window length (default 512; 1024 with --model newrale)")
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
    adapter = args.model == "newrale"
    L, ov = args.L or (1024 if adapter else 512), args.overlap
    hop = L - ov
    leads = 12 if adapter else 2
    streams = [int(v) for v in args.streams.split(",")]
    cmuls = [int(v) for v in args.cmul.split(",")]
    m = RALENet("full", leads=2, L=L, max_batch=4096, train=False, device=DEV, seed=1).eval()
    if adapter:
        m = NewRALE(m, seed=2).eval()
    Smax = max(streams)
    T = max(args.offline_T, 4 * max(cmuls) * hop)
    sig = _signal(Smax, T, leads).to(DEV)
    res = {"tool": "live_bench", "model": args.model, "leads": leads, "L": L, "overlap": ov, "hop": hop, "fs": FS, "legs": []}
    res["offline"] = _offline(m, sig, ov, args.reps)
    torch.cuda.empty_cache()
    for S in streams:
        for cm in cmuls:
            for mode in args.modes.split(","):
                res["legs"].append(_live_leg(m, sig, S, cm * hop, ov, mode == "graph", args.pushes))
                torch.cuda.empty_cache()
    off = res["offline"]["windows_per_s"]
    for leg in res["legs"]:
        leg["vs_offline"] = leg["windows_per_s"] / off
    if adapter and Smax >= 4096:
        res["unfused"] = _unfused_leg(m, sig, 4096, hop, ov, args.pushes)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
