"""Inference path: hipGraph-captured forward + streaming of long records (SURVEY §8f rank 3;
BASELINE config 4: 30-minute records, batches of 4096 windows, one MI355X).

The reference only has non-overlapping fixed-length chunking of the 650 000-sample MIT-BIH records
(local_utils/local_utils.py:116-130, 256-sample chunks, z-score per chunk group).  Here a record is cut
into windows of the model's length with an optional overlap; every window is z-scored per lead
(np_norm, local_utils/local_utils.py:261-266), denoised in eval mode (BatchNorm running statistics),
de-normalised and stitched back (overlapping regions keep the centre of each window).

A 12-lead `NewRALE` streams the same way around its inner 2-lead RA-LENet: the adapter convolutions run fused with the
windowing (`ral_newrale_stream_front`) and with the stitching (`ral_newrale_stream_back`).  Its captured plans remember the
model's parameter generation and are captured again once the weights change (the inner eval-mode forward leaves the
preparation of its weight planes out of a capture).

`LiveDenoiser` denoises S streams that arrive chunk by chunk, `NewRALELiveDenoiser` S 12-lead streams through a `NewRALE`;
what they return, concatenated, is what `StreamingDenoiser` returns for the complete records.  `LivePool` and
`NewRALELivePool` do the same for streams that start, stop and arrive independently of each other."""
import numpy as np
import torch

from . import _lib
from .model import NewRALE, _ptr, _stream
from .pools import SlotState, StreamSurface, as_chunks, pack_chunks, table_buffer


class GraphedForward:
    """model(x) for a fixed batch size captured once into a hipGraph (torch.cuda.CUDAGraph drives the
    capture; all kernels inside are libralenet launches on the capture stream and its forked lanes).

    With a `NewRALE` (12 leads in and out) a call captures again when the model's parameter generation has moved since the
    capture; it replays the eval-mode forward and refuses to run while the model is in training mode."""

    def __init__(self, model, batch):
        self.adapter = isinstance(model, NewRALE)      # 12 leads in and out, the inner engine sets L, device, max_batch
        e = model.rale.eng if self.adapter else model.eng
        if batch > e.max_batch:
            raise _lib.RalError(f"batch {batch} > max_batch {e.max_batch}")
        self.model, self.batch = model, batch
        model.eval()
        self.x = torch.zeros(batch, 12 if self.adapter else e.leads, e.L, dtype=torch.float32, device=e.device)
        self._capture()

    def _capture(self):
        model, e = self.model, (self.model.rale.eng if self.adapter else self.model.eng)
        self.gen = model.generation() if self.adapter else None
        side = torch.cuda.Stream(device=e.device)
        side.wait_stream(torch.cuda.current_stream(e.device))
        with torch.cuda.stream(side):          # warm-up outside capture (lazy LDS-size attributes, lanes)
            for _ in range(2):
                self.y = model(self.x)
        torch.cuda.current_stream(e.device).wait_stream(side)
        torch.cuda.synchronize(e.device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.y = model(self.x)

    def __call__(self, x):
        if self.adapter:
            if self.model.training:      # (a re-capture would need the eval forward: the caller's mode is not changed here)
                raise _lib.RalError("GraphedForward(NewRALE) replays the eval-mode forward: call model.eval() first")
            if self.model.generation() != self.gen:   # weights changed since the capture
                self._capture()
        self.x.copy_(x)
        self.graph.replay()
        return self.y


class StreamingDenoiser:
    """Long records through the eval-mode forward, everything on the device: `ral_stream_windows` (window gather +
    per-window z-score, statistics kept in a side buffer), the model in batches of `batch` windows, `ral_stream_stitch`
    (de-normalise + keep-the-centre stitching).  With `use_graph` the whole pipeline of a record group of a given
    shape (R, leads, T) is ONE hipGraph: replaying it costs one launch per group.

    A `NewRALE` streams 12-lead records (L and the batch cap from its inner engine): per batch of windows
    `ral_newrale_stream_front` (windows + z-score + conv1 + conv2), the inner eval forward, `ral_newrale_stream_back` (conv3 +
    conv4 + de-normalisation, written into the record).  Its plans are rebuilt when the model's parameter generation moves."""

    def __init__(self, model, batch=4096, overlap=0, use_graph=True, max_plans=4):
        self.adapter = isinstance(model, NewRALE)
        self.eng = model.rale.eng if self.adapter else model.eng      # the engine that runs the windows
        self.model, self.L, self.leads = model, self.eng.L, 12 if self.adapter else self.eng.leads
        self.max_plans = max(1, int(max_plans))      # plans (buffers + hipGraph per record-group shape) kept, LRU
        self.batch = min(batch, self.eng.max_batch)
        if overlap < 0 or overlap >= self.L or overlap % 2:
            raise _lib.RalError("overlap must be an even number of samples in [0, L)")
        self.overlap, self.hop = overlap, self.L - overlap
        self.use_graph = use_graph
        self.plans = {}
        model.eval()

    def windows_per_record(self, T):
        if T < self.L:
            raise _lib.RalError(f"record shorter than one window ({T} < {self.L})")
        n_reg = (T - self.L) // self.hop + 1
        return n_reg + (1 if (T - self.L) % self.hop else 0)

    def window_starts(self, T):
        n_reg = (T - self.L) // self.hop + 1
        st = [k * self.hop for k in range(n_reg)]
        return st + ([T - self.L] if (T - self.L) % self.hop else [])

    def _run(self, p):
        """enqueue the pipeline of one record group on the current stream (captured or eager)"""
        if self.adapter:
            return self._run_adapter(p)
        lib, e = _lib.lib(), self.model.eng
        R, T, nw_all = p["R"], p["T"], p["nw"]
        for w0 in range(0, nw_all, self.batch):
            nw = min(self.batch, nw_all - w0)
            _lib.check(lib.ral_stream_windows(_ptr(p["rec"]), R, T, self.leads, self.L, self.hop, w0, nw, _ptr(p["win"]),
                                              _ptr(p["stats"]), _stream()))
            _lib.check(lib.ral_forward(e.h, _ptr(p["win"]), _ptr(p["y"][w0:]), nw, 0, _stream()))
        _lib.check(lib.ral_stream_stitch(_ptr(p["y"]), _ptr(p["stats"]), R, T, self.leads, self.L, self.hop, _ptr(p["out"]),
                                         _stream()))

    def _run_adapter(self, p):
        lib, h, prm = _lib.lib(), self.eng.h, _ptr(self.model.params)
        R, T, nw_all = p["R"], p["T"], p["nw"]
        for w0 in range(0, nw_all, self.batch):
            nw = min(self.batch, nw_all - w0)
            _lib.check(lib.ral_newrale_stream_front(_ptr(p["rec"]), R, T, self.L, self.hop, w0, nw, prm, _ptr(p["win"]),
                                                    _ptr(p["stats"]), _stream()))
            _lib.check(lib.ral_forward(h, _ptr(p["win"]), _ptr(p["y"]), nw, 0, _stream()))
            _lib.check(lib.ral_newrale_stream_back(_ptr(p["y"]), _ptr(p["stats"]), prm, R, T, self.L, self.hop, w0, nw,
                                                   _ptr(p["out"]), _stream()))

    def _plan(self, R, T):
        key = (R, T)
        if self.adapter and key in self.plans and self.plans[key]["gen"] != self.model.generation():
            del self.plans[key]                         # captured under other weights
        if key in self.plans:
            self.plans[key] = self.plans.pop(key)       # most recently used last
            return self.plans[key]
        while len(self.plans) >= self.max_plans:        # drop the least recently used shape (its buffers and graph)
            self.plans.pop(next(iter(self.plans)))
        dev = self.eng.device
        nw = R * self.windows_per_record(T)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        if self.adapter:      # the inner model's input and output for one batch of windows
            nb = min(self.batch, nw)
            p = {"R": R, "T": T, "nw": nw, "rec": z(R, 12, T), "win": z(nb, 2, self.L), "y": z(nb, 2, self.L),
                 "stats": z(nw * 12 * 2), "out": z(R, 12, T), "graph": None, "gen": self.model.generation()}
        else:
            p = {"R": R, "T": T, "nw": nw, "rec": z(R, self.leads, T), "win": z(min(self.batch, nw), self.leads, self.L),
                 "y": z(nw, self.leads, self.L), "stats": z(nw * self.leads * 2), "out": z(R, self.leads, T), "graph": None}
        if self.use_graph:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):          # warm-up outside capture (lazy LDS-size attributes, lane streams)
                self._run(p)
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            p["graph"] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(p["graph"]):
                self._run(p)
        self.plans[key] = p
        return p

    @torch.no_grad()
    def denoise(self, record, copy=True):
        """record: (leads, T) or a group (R, leads, T), host or device -> denoised record(s) of the same shape on the
        device.  The result is a fresh tensor; `copy=False` returns a view of the plan's output buffer instead, which the
        next call with the same shape overwrites (throughput loops that consume each result before the next call)."""
        dev = self.eng.device
        rec = torch.as_tensor(record, dtype=torch.float32)
        single = rec.dim() == 2
        if single:
            rec = rec[None]
        if rec.dim() != 3 or rec.shape[1] != self.leads:
            raise _lib.RalError(f"expected a record of shape ({self.leads}, T) or (R, {self.leads}, T)")
        p = self._plan(rec.shape[0], rec.shape[2])
        p["rec"].copy_(rec, non_blocking=True)
        if p["graph"] is not None:
            p["graph"].replay()
        else:
            self._run(p)
        out = p["out"][0] if single else p["out"]
        return out.clone() if copy else out

    def evaluate(self, records, noise, snr_db, offsets=None, rng=None, window=None):
        """Noise-stress evaluation of a record group on the device: clean `records` (R, leads, T) and one noise record
        `noise` (leads, Tn), device tensors -> `evaluate.RecordScores`.  `mix_records` z-scores every record and adds its noise
        segment at `snr_db` dB (a scalar or one value per record: a whole intensity sweep in one call), the noisy records are
        streamed through `denoise`, and `score_records` gives SNR in / out and RMSE in / out per lead, per record, per tile of
        `window` samples (default L) and as tile means.  The plans and graphs of `denoise` are used as they are."""
        from .evaluate import mix_records, score_records
        if not torch.is_tensor(records) or records.dim() != 3 or records.shape[1] != self.leads:
            raise _lib.RalError(f"evaluate: expected a device tensor of records of shape (R, {self.leads}, T)")
        noisy, clean = mix_records(records, noise, snr_db, offsets, rng)
        out = self.denoise(noisy, copy=False)
        return score_records(clean, out, noisy, self.L if window is None else window)


def live_frontier(n, L, hop):
    """F(n): after n samples of a stream, samples [0, F(n)) are final for every length T >= n the stream may end at.  Each is
    kept by a regular window that is complete at n (window k keeps [k hop + h, (k + 1) hop + h), window 0 from 0; h =
    (L - hop) / 2), and neither a later window nor the right-aligned last one of any T >= n claims it.  0 before the first
    window is complete."""
    if n < L:
        return 0
    return ((n - L) // hop + 1) * hop + (L - hop) // 2


def live_latency(L, hop):
    """D = n - F(n) for every n >= L on the hop grid: the constant lag of a live stream fed in chunks of a multiple of hop"""
    return (-L) % hop + (L - hop) // 2


class _LiveBase:
    """What the live denoisers share: the stream geometry, the frontier bookkeeping of `push` / `flush`, the two hipGraphs of
    the steady state (one per push parity) and their capture.  A subclass allocates its buffers and supplies `_run` (one call:
    the windows of every stream, the model, the kept samples) and `_emit_last` (at `flush`, the samples the last regular window
    of the pushes keeps)."""

    def _setup(self, model, eng, leads, streams, chunk, overlap, use_graph):
        """validate and set the geometry -> windows per stream and push, at most (every push once the lag is constant)"""
        self.model, self.eng, self.L, self.leads = model, eng, eng.L, leads
        if overlap < 0 or overlap >= self.L or overlap % 2:
            raise _lib.RalError("overlap must be an even number of samples in [0, L)")
        self.overlap, self.hop = overlap, self.L - overlap
        if streams < 1:
            raise _lib.RalError("streams must be >= 1")
        if chunk < 1 or chunk % self.hop:
            raise _lib.RalError(f"chunk must be a positive multiple of hop = L - overlap = {self.hop} (got {chunk})")
        self.S, self.C, self.use_graph = int(streams), int(chunk), use_graph
        self.graphs, self.gen = [None, None], None
        self.latency = live_latency(self.L, self.hop)
        return self.C // self.hop

    def reset(self):
        """drop every stream's state; the next push starts new streams (the captured graphs stay valid)"""
        self.samples_in, self.parity = 0, 0

    def _n_reg(self, n):
        return (n - self.L) // self.hop + 1 if n >= self.L else 0

    def _generation(self):
        """the parameter generation the captured graphs are valid for"""
        return self.model.param_gen

    def _ready(self, what):
        """raise if the model cannot run a live call now"""

    def _chunk(self, x, what):
        x = torch.as_tensor(x, dtype=torch.float32)
        if x.dim() != 3 or x.shape[0] != self.S or x.shape[1] != self.leads:
            raise _lib.RalError(f"{what}: expected a chunk of shape ({self.S}, {self.leads}, samples), got {tuple(x.shape)}")
        return x

    def _capture(self, args):
        dev = self.eng.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):          # warm-up outside capture (lazy LDS-size attributes, lane streams)
            self._run(*args)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._run(*args)
        return g

    @torch.no_grad()
    def push(self, x, copy=True):
        """x (S, leads, C), host or device -> the samples of every stream that became final, (S, leads, m) on the device.  The
        result is a fresh tensor; `copy=False` returns a view of a buffer that the next push may overwrite."""
        self._ready("push")
        x = self._chunk(x, "push")
        if x.shape[2] != self.C:
            raise _lib.RalError(f"push: every chunk has C = {self.C} samples (got {x.shape[2]}); flush takes a shorter last one")
        n0, n1 = self.samples_in, self.samples_in + self.C
        k0 = self._n_reg(n0)
        nw = self._n_reg(n1) - k0
        lo = live_frontier(n0, self.L, self.hop)
        m = live_frontier(n1, self.L, self.hop) - lo
        self.x.copy_(x, non_blocking=True)
        if n0 >= self.L and self.use_graph:
            # steady state: nw = C / hop, m = C, k0 > 0; the arguments of the capturing push serve every later push of the
            # same parity (the open-stream rule depends only on positions relative to the history)
            gen = self._generation()
            if self.gen != gen:
                self.graphs, self.gen = [None, None], gen
            if self.graphs[self.parity] is None:
                self.graphs[self.parity] = self._capture((self.x, self.C, k0, nw, -1, lo, m, self.out, True, self.stats))
            self.graphs[self.parity].replay()
            out = self.out
        else:
            out = self.out if m == self.C else torch.empty(self.S, self.leads, m, device=self.eng.device)
            self._run(self.x, self.C, k0, nw, -1, lo, m, out, True, self.stats)
        self.samples_in, self.parity = n1, 1 - self.parity
        return out.clone() if copy and out is self.out else out

    @torch.no_grad()
    def flush(self, x=None):
        """the optional last chunk x (S, leads, r), any r >= 0 -> the rest of every stream, (S, leads, T - F(n)) for a stream of
        T = n + r samples; the object is reset afterwards"""
        self._ready("flush")
        r = 0 if x is None else self._chunk(x, "flush").shape[2]
        n, T = self.samples_in, self.samples_in + r
        if T < self.L:
            raise _lib.RalError(f"flush: a stream shorter than one window ({T} < {self.L} samples)")
        xd = torch.zeros(self.S, self.leads, max(r, 1), device=self.eng.device)
        if r:
            xd.copy_(x)
        k0 = self._n_reg(n)
        nw = (T - self.L) // self.hop + 1 + (1 if (T - self.L) % self.hop else 0) - k0
        lo = live_frontier(n, self.L, self.hop)
        out = torch.empty(self.S, self.leads, T - lo, device=self.eng.device)
        if nw:   # (a long last chunk may hold more windows than a push: stats of their own)
            stats = self.stats if self.stats.numel() >= self.S * nw * self.leads * 2 else \
                torch.empty(self.S * nw * self.leads * 2, device=self.eng.device)
            self._run(xd, r, k0, nw, T, lo, T - lo, out, False, stats)
        if n >= self.L and T > lo:    # the last regular window of the pushes: it keeps [lo, T) if it is the stream's last one
            self._emit_last(k0 - 1, T, lo, out)
        self.reset()
        return out


class LiveDenoiser(_LiveBase):
    """S streams denoised while they arrive, in lockstep chunks of C samples (C a positive multiple of hop = L - overlap).

    `push(x)` takes the next chunk of every stream, x (S, leads, C), and returns the samples that have become final, (S, leads,
    m) on the device: nothing before L samples have arrived, samples [0, F(n)) when the first window completes
    (`live_frontier`), then C per push, `latency` samples behind the newest one.  `flush(x=None)` takes an optional last chunk of
    any length r >= 0, returns the rest of every stream and resets the object.  Concatenated per stream, everything `push` and
    `flush` returned equals `StreamingDenoiser(model, overlap=overlap).denoise(record)`: the same windows, per-window z-score,
    stitch rule and right-aligned last window.

    Per push `ral_live_windows` gathers every stream's new windows straight from its last L samples (kept on the device, two
    buffers used in turn: a push reads one and writes the other) and the chunk, the model runs them in batches of at most
    max_batch windows, and `ral_live_emit` writes the samples they keep.  Once the lag is constant (the first L samples have
    arrived) a push replays one of two captured hipGraphs, by push parity; they are captured again when the model's parameter
    generation moves (the eval-mode capture leaves out the preparation of the weight planes).  Earlier pushes and `flush` run
    eagerly.  Accepts the 1- and 2-lead models of `StreamingDenoiser` (RALENet, UNet, ACDAE, DANet); puts the model in eval mode.
    A 12-lead `NewRALE` streams through `NewRALELiveDenoiser`."""

    def __init__(self, model, streams, chunk, overlap=0, use_graph=True):
        if isinstance(model, NewRALE):
            raise _lib.RalError("LiveDenoiser does not take a NewRALE: live 12-lead streams run through NewRALELiveDenoiser")
        e = model.eng
        nw = self._setup(model, e, e.leads, streams, chunk, overlap, use_graph)
        dev = e.device
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.hist = [z(self.S, self.leads, self.L), z(self.S, self.leads, self.L)]    # push parity p reads hist[p], writes hist[1 - p]
        self.x = z(self.S, self.leads, self.C)
        self.win = z(min(e.max_batch, self.S * nw), self.leads, self.L)      # one batch of windows
        self.y = torch.zeros_like(self.win)
        self.stats = z(self.S * nw * self.leads * 2)
        self.out = z(self.S, self.leads, self.C)
        self.last_y, self.last_stats = z(self.S, self.leads, self.L), z(self.S * self.leads * 2)   # the last regular window
        model.eval()
        self.reset()

    def _run(self, x, C, k0, nw, T, lo, m, out, keep, stats):
        """enqueue one call on the current stream (captured or eager): the windows k0 .. k0 + nw - 1 of every stream from the
        history and x (C samples), the model, the kept samples in [lo, lo + m) -> out; a push (keep) also writes the next
        history and keeps the last window.  stats: (mean, std) of the S * nw windows"""
        lib, e, S, n = _lib.lib(), self.eng, self.S, self.samples_in
        h_in, h_out = self.hist[self.parity], (self.hist[1 - self.parity] if keep else None)
        base, batch = n - self.L, self.win.shape[0]
        for w0 in range(0, max(S * nw, 1), batch):
            nb = min(batch, S * nw - w0)
            if nb == 0 and h_out is None:
                break
            _lib.check(lib.ral_live_windows(_ptr(h_in), _ptr(x), _ptr(h_out if w0 == 0 else None), S, self.leads, self.L,
                                            self.hop, C, base, k0, nw, T, w0, nb, _ptr(self.win), _ptr(stats), _stream()))
            if nb == 0:
                break
            _lib.check(lib.ral_forward(e.h, _ptr(self.win), _ptr(self.y), nb, 0, _stream()))
            _lib.check(lib.ral_live_emit(_ptr(self.y), _ptr(stats), S, self.leads, self.L, self.hop, k0, nw, T, w0, nb, lo,
                                         m, _ptr(out), _ptr(self.last_y if keep else None),
                                         _ptr(self.last_stats if keep else None), _stream()))

    def _emit_last(self, k, T, lo, out):
        _lib.check(_lib.lib().ral_live_emit(_ptr(self.last_y), _ptr(self.last_stats), self.S, self.leads, self.L, self.hop,
                                            k, 1, T, 0, self.S, lo, T - lo, _ptr(out), None, None, _stream()))


class NewRALELiveDenoiser(_LiveBase):
    """`LiveDenoiser` for a 12-lead `NewRALE`: S streams of 12 leads denoised while they arrive, in lockstep chunks of C samples
    (a positive multiple of hop = L - overlap; L from the inner model).  The same surface and contract: `push(x)` with x
    (S, 12, C), `flush(x=None)`, `reset()`, `latency`; concatenated per stream, what they return equals
    `StreamingDenoiser(model, overlap=overlap).denoise(record)`.

    Per batch of at most max_batch windows (of the inner engine) `ral_newrale_live_front` gathers every stream's new windows
    from its history and the chunk, z-scores them per lead and applies conv1 and conv2 (its first launch of a push also writes
    the next history), the inner model runs its eval-mode forward, and `ral_newrale_live_back` applies conv3 and conv4,
    de-normalises and writes the kept samples.  The steady-state graphs are captured again when `model.generation()` (adapter,
    inner model) moves.  `push` and `flush` refuse a model in training mode (the inner BatchNorm would use batch statistics);
    the constructor puts the model in eval mode."""

    def __init__(self, model, streams, chunk, overlap=0, use_graph=True):
        if not isinstance(model, NewRALE):
            raise _lib.RalError(f"NewRALELiveDenoiser takes a NewRALE (got {type(model).__name__}; LiveDenoiser takes the "
                                "1- and 2-lead models)")
        e = model.rale.eng
        nw = self._setup(model, e, 12, streams, chunk, overlap, use_graph)
        dev = e.device
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.hist = [z(self.S, 12, self.L), z(self.S, 12, self.L)]    # push parity p reads hist[p], writes hist[1 - p]
        self.x = z(self.S, 12, self.C)
        self.win = z(min(e.max_batch, self.S * nw), 2, self.L)      # the inner model's input and output for one batch
        self.y = torch.zeros_like(self.win)
        self.stats = z(self.S * nw * 12 * 2)
        self.out = z(self.S, 12, self.C)
        self.last_y, self.last_stats = z(self.S, 2, self.L), z(self.S * 12 * 2)   # the last regular window (inner output)
        model.eval()
        self.reset()

    def _generation(self):
        return self.model.generation()

    def _ready(self, what):
        if self.model.training:
            raise _lib.RalError(f"NewRALELiveDenoiser.{what} runs the eval-mode forward: call model.eval() first")

    def _run(self, x, C, k0, nw, T, lo, m, out, keep, stats):
        """as LiveDenoiser._run, through the adapter kernels around the inner model"""
        lib, h, S, n = _lib.lib(), self.eng.h, self.S, self.samples_in
        prm = _ptr(self.model.params)
        h_in, h_out = self.hist[self.parity], (self.hist[1 - self.parity] if keep else None)
        base, batch = n - self.L, self.win.shape[0]
        for w0 in range(0, max(S * nw, 1), batch):
            nb = min(batch, S * nw - w0)
            if nb == 0 and h_out is None:
                break
            _lib.check(lib.ral_newrale_live_front(_ptr(h_in), _ptr(x), _ptr(h_out if w0 == 0 else None), S, self.L, self.hop, C,
                                                  base, k0, nw, T, w0, nb, prm, _ptr(self.win), _ptr(stats), _stream()))
            if nb == 0:
                break
            _lib.check(lib.ral_forward(h, _ptr(self.win), _ptr(self.y), nb, 0, _stream()))
            _lib.check(lib.ral_newrale_live_back(_ptr(self.y), _ptr(stats), prm, S, self.L, self.hop, k0, nw, T, w0, nb, lo, m,
                                                 _ptr(out), _ptr(self.last_y if keep else None),
                                                 _ptr(self.last_stats if keep else None), _stream()))

    def _emit_last(self, k, T, lo, out):
        _lib.check(_lib.lib().ral_newrale_live_back(_ptr(self.last_y), _ptr(self.last_stats), _ptr(self.model.params), self.S,
                                                    self.L, self.hop, k, 1, T, 0, self.S, lo, T - lo, _ptr(out), None, None,
                                                    _stream()))


def pool_plan(n0, c, closing, L, hop):
    """What one call does for a stream that had received n0 samples and now gets c more (closing: the stream ends with them, and
    n0 + c >= L) -> (first window k0, window count nw, lo, m, T): the call runs windows k0 .. k0 + nw - 1 of the stream, emits
    samples [lo, lo + m), and T is the stream's length (-1 while it stays open).  An open stream runs the regular windows that
    became complete and emits up to `live_frontier(n0 + c)`; a closing one runs all remaining windows (the right-aligned last
    one among them) and emits up to its end.  A pure function of its arguments, elementwise over integers or integer arrays."""
    n0, c = np.asarray(n0, dtype=np.int64), np.asarray(c, dtype=np.int64)
    closing = np.asarray(closing, dtype=bool)
    n1, h = n0 + c, (L - hop) // 2
    n_reg = lambda n: np.where(n >= L, (n - L) // hop + 1, 0)
    front = lambda n: np.where(n >= L, n_reg(n) * hop + h, 0)
    k0, lo = n_reg(n0), front(n0)
    n_all = n_reg(n1) + ((n1 - L) % hop != 0)           # every window of a stream of n1 samples
    nw = np.where(closing, n_all, n_reg(n1)) - k0
    m = np.where(closing, n1, front(n1)) - lo
    return k0, nw, lo, m, np.where(closing, n1, -1)


class PoolState(SlotState):
    """The host side of a stream pool, without a device: the slots (`SlotState`) and the window geometry.  `plan` checks the
    arguments of a call and builds its tables (`_lib.POOL_ROW`) without changing anything; `commit` applies a planned call."""

    def __init__(self, capacity, leads, L, overlap, name="LivePool", grid=(64, 2048)):
        if L < grid[0] or L % grid[0] or L > grid[1]:      # the window lengths of the pool's gather / emit kernels
            raise _lib.RalError(f"{name}: L must be a multiple of {grid[0]} up to {grid[1]} (got {L})")
        if overlap < 0 or overlap >= L or overlap % 2:
            raise _lib.RalError("overlap must be an even number of samples in [0, L)")
        super().__init__(capacity, leads, name)
        self.L, self.hop = int(L), int(L - overlap)

    def plan(self, shapes, close=()):
        """shapes {sid: shape of its chunk}, close: the sids that end with this call -> (sids in row order, table, table of the
        kept last windows to emit); raises RalError for a bad argument"""
        name = self.name
        named = self.named(shapes, close)
        sids, _, lens, ends, n0 = named
        if np.any((lens == 0) & ~ends):
            sid = sids[int(np.argmax((lens == 0) & ~ends))]
            raise _lib.RalError(f"{name}.push: stream {sid}: an empty chunk (only a closing stream may come without samples)")
        short = ends & (n0 + lens < self.L)
        if np.any(short):
            r = int(np.argmax(short))
            raise _lib.RalError(f"{name}.push: stream {sids[r]} would end shorter than one window ({int(n0[r] + lens[r])} < "
                                f"{self.L} samples)")
        k0, nw, lo, m, T = pool_plan(n0, lens, ends, self.L, self.hop)
        tab = self.rows(_lib.POOL_ROW, named)            # (T as pool_plan gives it)
        tab["k0"], tab["lo"], tab["nw"], tab["m"] = k0, lo, nw, m
        tab["out_off"], tab["w_off"] = np.cumsum(m) - m, np.cumsum(nw) - nw
        # a closing stream without a further window: its last regular window so far turns out to be its last one and keeps
        # [lo, T) (with further windows that one stays regular and has given everything it keeps)
        last = tab[ends & (n0 >= self.L) & (nw == 0) & (T > lo)].copy()
        last["k0"] -= 1
        last["nw"], last["w_off"] = 1, np.arange(len(last))
        return sids, tab, last

    commit = SlotState.commit_rows


class _PoolBase(StreamSurface):
    """What the window pools share: the slots and their state (`PoolState`), the batches of at most max_batch windows, the packed
    result; `close(sid, x=None)` returns the rest of a stream, (leads, T - F(n)).  A subclass supplies the model check, `_gather`
    and `_emit`."""

    def _setup(self, model, eng, leads, inner_leads, capacity, overlap, grid):
        self.model, self.eng, self.leads = model, eng, leads
        self.state = PoolState(capacity, leads, eng.L, overlap, type(self).__name__, grid)
        self.capacity, self.L, self.hop, self.overlap = self.state.capacity, eng.L, self.state.hop, overlap
        dev = eng.device
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.hist = z(2, self.capacity, leads, self.L)        # a slot reads plane turn[slot] and writes the other
        self.last_y, self.last_stats = z(self.capacity, inner_leads, self.L), z(self.capacity, leads, 2)
        self.inner_leads = inner_leads
        self.win = self.y = self.stats = None                  # one batch of windows, the call's statistics: grown on demand
        self.windows_run = 0                                   # windows the pool has run so far
        model.eval()

    def _ready(self, what):
        """raise if the model cannot run a call now"""

    @torch.no_grad()
    def push(self, chunks, close=()):
        """chunks {sid: (leads, c) samples, host or device}, close: the sids that end with this call (with or without a chunk) ->
        {sid: the samples that became final, (leads, m) on the device} for every sid named.  Every argument is checked before any
        device work; a call that raises has changed nothing."""
        self._ready("push")
        dev = self.eng.device
        xs = as_chunks(chunks)
        sids, tab, last = self.state.plan({sid: tuple(x.shape) for sid, x in xs.items()}, tuple(close))
        lib, leads, R = _lib.lib(), self.leads, len(tab)
        out_total, total = int(tab["m"].sum()), int(tab["w_off"][-1] + tab["nw"][-1])
        xp, x_total, _ = pack_chunks(xs, leads, dev)
        out = torch.empty(max(out_total, 1) * leads, dtype=torch.float32, device=dev)
        batch = min(self.eng.max_batch, max(total, 1))
        if self.win is None or self.win.shape[0] < batch:
            self.win = torch.zeros(batch, self.inner_leads, self.L, dtype=torch.float32, device=dev)
            self.y = torch.zeros_like(self.win)
        if self.stats is None or self.stats.numel() < total * leads * 2:
            self.stats = torch.zeros(max(total, 1) * leads * 2, dtype=torch.float32, device=dev)
        tab_dev = table_buffer(tab, dev)
        geom = (self.capacity, leads, self.L, self.hop)
        keep_any, first = bool((tab["flags"] & _lib.POOL_KEEP).any()), True
        for w0 in range(0, max(total, 1), self.win.shape[0]):
            nb = min(self.win.shape[0], total - w0)
            write_hist = first and keep_any          # the call's first gather also writes the next histories
            if nb == 0 and not write_hist:
                break
            self._gather(lib, xp, x_total, tab, tab_dev, first, geom, write_hist, w0, nb)
            first = False
            if nb == 0:
                break
            _lib.check(lib.ral_forward(self.eng.h, _ptr(self.win), _ptr(self.y), nb, 0, _stream()))
            self._emit(lib, self.y, self.stats, tab, tab_dev, False, geom, w0, nb, False, out, out_total, True)
        if len(last):
            last_dev = table_buffer(last, dev)
            self._emit(lib, self.last_y, self.last_stats, last, last_dev, True, geom, 0, len(last), True, out, out_total, False)
        self.state.commit(tab)
        self.windows_run += total
        parts = out[:out_total * leads].split([int(v) * leads for v in tab["m"]])
        return {sid: p.view(leads, -1) for sid, p in zip(sids, parts)}


class LivePool(_PoolBase):
    """A pool of up to `capacity` independent live streams: each is opened and closed on its own and gets chunks of any length,
    whenever they come.  `open()` returns a stream id; `push(chunks, close=())` takes {sid: (leads, c)} for any subset of the
    open streams, ends the streams listed in `close`, and returns {sid: (leads, m)} on the device, the samples of each named
    stream that became final: after n samples a stream has been given exactly [0, live_frontier(n, L, hop)), and closing it
    returns the rest.  Concatenated per stream from `open` to `close`, the results equal
    `StreamingDenoiser(model, overlap=overlap).denoise(record)` on the complete record bit for bit, whatever the chunking, the
    other streams of the pool, the slot and the batching.  `close(sid, x=None)` ends one stream.

    Per call the host plans one table row per named stream (`pool_plan`), `ral_pool_windows` gathers every window that became
    complete from the slots' last L samples and the packed chunks (its first launch also writes the next history of the rows
    that stay open, into the slot's other buffer), the model runs them in batches of at most max_batch windows in eval mode,
    and `ral_pool_emit` writes the samples they keep into one packed result.  No hipGraph: the geometry differs from call to
    call, so every call runs the ordinary eval forward and weight changes take effect at once.  Accepts the 1- and 2-lead
    models of `LiveDenoiser` (RALENet, UNet, ACDAE, DANet); puts the model in eval mode.  A `NewRALE` runs through
    `NewRALELivePool`."""

    def __init__(self, model, capacity, overlap=0):
        if isinstance(model, NewRALE):
            raise _lib.RalError("LivePool does not take a NewRALE: pools of 12-lead streams run through NewRALELivePool")
        self._setup(model, model.eng, model.eng.leads, model.eng.leads, capacity, overlap, (64, 2048))

    def _gather(self, lib, xp, x_total, tab, tab_dev, upload, geom, write_hist, w0, nb):
        cap, leads, L, hop = geom
        _lib.check(lib.ral_pool_windows(_ptr(self.hist), _ptr(xp), x_total, tab.ctypes.data, len(tab), _ptr(tab_dev), int(upload),
                                        cap, leads, L, hop, int(write_hist), w0, nb, _ptr(self.win), _ptr(self.stats), _stream()))

    def _emit(self, lib, y, stats, tab, tab_dev, upload, geom, w0, nb, from_last, out, out_total, keep):
        cap, leads, L, hop = geom
        _lib.check(lib.ral_pool_emit(_ptr(y), _ptr(stats), tab.ctypes.data, len(tab), _ptr(tab_dev), int(upload), cap, leads, L,
                                     hop, w0, nb, int(from_last), _ptr(out), out_total, _ptr(self.last_y if keep else None),
                                     _ptr(self.last_stats if keep else None), _stream()))


class NewRALELivePool(_PoolBase):
    """`LivePool` for a 12-lead `NewRALE`: the same surface and contract with chunks of shape (12, c).  Per batch
    `ral_newrale_pool_front` gathers the windows, z-scores every lead and applies conv1 and conv2, the inner model runs its
    eval-mode forward, and `ral_newrale_pool_back` applies conv3 and conv4, de-normalises and writes the kept samples; the kept
    last window of a slot is the inner output.  `push` and `close` refuse a model in training mode; the constructor puts the
    model in eval mode."""

    def __init__(self, model, capacity, overlap=0):
        if not isinstance(model, NewRALE):
            raise _lib.RalError(f"NewRALELivePool takes a NewRALE (got {type(model).__name__}; LivePool takes the 1- and 2-lead "
                                "models)")
        self._setup(model, model.rale.eng, 12, 2, capacity, overlap, (16, 1024))

    def _ready(self, what):
        if self.model.training:
            raise _lib.RalError(f"NewRALELivePool.{what} runs the eval-mode forward: call model.eval() first")

    def _gather(self, lib, xp, x_total, tab, tab_dev, upload, geom, write_hist, w0, nb):
        cap, _, L, hop = geom
        _lib.check(lib.ral_newrale_pool_front(_ptr(self.hist), _ptr(xp), x_total, tab.ctypes.data, len(tab), _ptr(tab_dev),
                                              int(upload), cap, L, hop, int(write_hist), w0, nb, _ptr(self.model.params),
                                              _ptr(self.win), _ptr(self.stats), _stream()))

    def _emit(self, lib, y, stats, tab, tab_dev, upload, geom, w0, nb, from_last, out, out_total, keep):
        cap, _, L, hop = geom
        _lib.check(lib.ral_newrale_pool_back(_ptr(y), _ptr(stats), _ptr(self.model.params), tab.ctypes.data, len(tab),
                                             _ptr(tab_dev), int(upload), cap, L, hop, w0, nb, int(from_last), _ptr(out), out_total,
                                             _ptr(self.last_y if keep else None), _ptr(self.last_stats if keep else None),
                                             _stream()))
