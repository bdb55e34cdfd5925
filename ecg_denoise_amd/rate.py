"""Sample-rate conversion on the device: records and live streams sampled at another rate than the model's 360 Hz.

Every model here is trained at the MIT-BIH rate; `StreamingDenoiser`, `LivePool` and the other inference entry points take
their samples at that rate.  This module converts in front of and behind them:

    Resampler(500, 360, device).convert(x)             # whole records, ral_rate_records
    ResamplerPool(500, 360, leads, capacity, device)   # chunks of independent streams, ral_rate_pool
    RateStreamingDenoiser(model, fs=500)               # convert -> StreamingDenoiser -> convert back
    RateLivePool(model, fs=500, capacity=64)           # ResamplerPool -> LivePool / NewRALELivePool -> ResamplerPool

The conversion (include/ralenet.h has the same definition) is that of
`scipy.signal.resample_poly(x, up, down, window=('kaiser', 5.0), padtype='edge')`, up / down = fs_out / fs_in in lowest terms:

    mx = max(up, down); half = 10 * mx; k = -half .. half
    h[k + half] = (1 / mx) * sinc(k / mx) * np.kaiser(2 * half + 1, 5.0)[k + half];   h *= up / h.sum()
    T_out = ceil(T * up / down)
    y[m] = sum over n = ceil((m * down - half) / up) .. floor((m * down + half) / up) of
           h[m * down - n * up + half] * x[clamp(n, 0, T - 1)]

The filter is designed here in fp64 with numpy (no scipy at run time); the device accumulates in fp32 with fmaf in ascending
n, so a stream converted chunk by chunk equals the converted record bit for bit.  Only the `edge` mode exists (the first and
the last sample are replicated): zero extension of an ADC signal with a baseline of 1024 would ring through the first windows.

`LiveDenoiser` (lockstep streams, a fixed chunk per push) has no counterpart here: a fixed chunk at the input rate is not a
fixed chunk at the model's rate, which is what its captured graphs need.  Lockstep streams at another rate go through
`RateLivePool`."""
import numbers
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from .infer import LivePool, NewRALELivePool, StreamingDenoiser
from .model import NewRALE, _ptr, _stream
from .pools import SlotState, StreamSurface, as_chunks, pack_chunks, table_buffer

MODEL_RATE = 360

# the LDS budget of ral_rate.hip (rate_geom there): a tile of at most _TILE_MAX outputs, halved down to _TILE_MIN while its
# input span exceeds _SPAN_CAP floats; the bank, the span and the tile must fit _LDS_FLOATS floats
_TILE_MAX, _TILE_MIN, _SPAN_CAP, _LDS_FLOATS = 1024, 64, 4096, 16384


def _rate(v, what):
    if isinstance(v, bool) or not isinstance(v, (numbers.Integral, Fraction, float, np.floating)):
        raise _lib.RalError(f"{what} must be a positive int or Fraction (got {v!r})")
    if isinstance(v, (float, np.floating)):
        if v != v or v in (float("inf"), float("-inf")) or v != int(v):
            raise _lib.RalError(f"{what} must be a positive int or Fraction: a float that is not integral is refused (got {v!r})")
        v = int(v)
    v = Fraction(v)
    if v <= 0:
        raise _lib.RalError(f"{what} must be positive (got {v})")
    return v


def rate_ratio(fs_in, fs_out):
    """-> (up, down), fs_out / fs_in in lowest terms.  Rates are positive ints or Fractions; a non-integral float is refused."""
    q = _rate(fs_out, "fs_out") / _rate(fs_in, "fs_in")
    return q.numerator, q.denominator


def _pair(up, down):
    for v in (up, down):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
            raise _lib.RalError(f"up and down must be positive ints (got up={up!r} down={down!r})")
    return int(up), int(down)


def rate_half(up, down):
    """half the filter length: the filter has 2 * half + 1 taps"""
    return 10 * max(_pair(up, down))


def rate_taps_per_output(up, down):
    """K = ceil((2 half + 1) / up): the taps one output sums (some outputs one fewer), and the samples a stream keeps"""
    return (2 * rate_half(up, down) + up) // up


def rate_check(up, down):
    """raise RalError unless the pair's bank and the input span of one tile of outputs fit the kernel's LDS budget"""
    up, down = _pair(up, down)
    if np.gcd(up, down) != 1:
        raise _lib.RalError(f"up / down must be in lowest terms (got up={up} down={down})")
    K = rate_taps_per_output(up, down)
    span = lambda tile: (tile - 1) * down // up + K + 2
    tile = _TILE_MAX
    while tile > _TILE_MIN and span(tile) > _SPAN_CAP:
        tile //= 2
    need = (K * up + 3) // 4 * 4 + (span(tile) + 8 + 3) // 4 * 4 + tile + 8
    if max(up, down) > 65535 or need > _LDS_FLOATS:
        raise _lib.RalError(f"rate conversion up={up} down={down} is not supported: its filter bank ({K * up} floats) and the "
                            f"input span of a tile do not fit the kernel's {_LDS_FLOATS * 4 // 1024} KB of LDS")
    return up, down


def rate_bank(up, down):
    """the 2 * half + 1 filter taps of up / down, fp64: firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up"""
    up, down = _pair(up, down)
    mx, half = max(up, down), rate_half(up, down)
    k = np.arange(-half, half + 1, dtype=np.float64)
    h = (1.0 / mx) * np.sinc(k / mx) * np.kaiser(2 * half + 1, 5.0)
    return h * (up / h.sum())


def rate_length(T, up, down):
    """samples a signal of T samples converts to: ceil(T up / down)"""
    return -((-int(T) * up) // down)


def rate_frontier(n, up, down):
    """outputs that are final once a stream has received n samples, whatever follows: output m is final iff
    m down + half < n up, so max(0, ceil((n up - half) / down))"""
    return max(0, -((rate_half(up, down) - int(n) * up) // down))


def rate_latency(fs_in, fs_out):
    """the input samples an output waits for after its own instant: half / up"""
    up, down = rate_ratio(fs_in, fs_out)
    return rate_half(up, down) / up


class Resampler:
    """Whole records from `fs_in` to `fs_out` on `device` (`ral_rate_records`).  `convert(x)` takes (leads, T) or (R, leads, T),
    host or device, and returns a device tensor at `fs_out` with T_out = `rate_length(T, up, down)` samples.  The filter bank is
    designed and uploaded once per instance.  With fs_in == fs_out nothing is converted: the data comes back untouched."""

    def __init__(self, fs_in, fs_out, device="cuda"):
        self.fs_in, self.fs_out = fs_in, fs_out
        self.up, self.down = rate_ratio(fs_in, fs_out)
        self.identity = self.up == self.down == 1
        self.device = torch.device(device)
        self.bank = None
        if not self.identity:
            rate_check(self.up, self.down)
            self.bank = torch.from_numpy(rate_bank(self.up, self.down).astype(np.float32)).to(self.device)

    def length(self, T):
        return int(T) if self.identity else rate_length(T, self.up, self.down)

    @torch.no_grad()
    def convert(self, x):
        x = torch.as_tensor(x)
        if x.dim() not in (2, 3) or x.shape[-1] < 1 or x.shape[-2] < 1:
            raise _lib.RalError(f"Resampler.convert: expected (leads, T) or (R, leads, T) with T >= 1, got {tuple(x.shape)}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if self.identity or x.shape[0] == 0:
            return x
        R, leads, T = (1,) + tuple(x.shape) if x.dim() == 2 else tuple(x.shape)
        T_out = rate_length(T, self.up, self.down)
        with torch.cuda.device(self.device):
            y = torch.empty(x.shape[:-1] + (T_out,), dtype=torch.float32, device=self.device)
            _lib.check(_lib.lib().ral_rate_records(_ptr(x), R, leads, T, self.up, self.down, _ptr(self.bank), self.bank.numel(),
                                                   _ptr(y), T_out, _stream()))
        return y


class RatePoolState(SlotState):
    """The host side of a `ResamplerPool`, without a device: the slots (`SlotState`) and the conversion.  `plan` checks the
    arguments of a call and builds its table (`_lib.RATE_ROW`) without changing anything; `commit` applies a planned call.
    After n samples a stream has been given `frontier(n)` outputs; closing it at T gives the rest, up to `length(T)`."""

    def __init__(self, up, down, leads, capacity, name="ResamplerPool"):
        self.up, self.down = _pair(up, down)
        self.identity = self.up == self.down == 1
        if not self.identity:
            rate_check(self.up, self.down)
        if not isinstance(leads, numbers.Integral) or leads < 1:
            raise _lib.RalError(f"{name}: leads must be >= 1")
        super().__init__(capacity, leads, name)
        self.hist_len = rate_taps_per_output(self.up, self.down)      # 2 half / up + 1

    def frontier(self, n):
        return int(n) if self.identity else rate_frontier(n, self.up, self.down)

    def length(self, T):
        return int(T) if self.identity else rate_length(T, self.up, self.down)

    def plan(self, shapes, close=()):
        """shapes {sid: shape of its chunk, (leads, c) with c >= 0}, close: the sids that end with this call -> (sids in row
        order, table); raises RalError for a bad argument"""
        named = self.named(shapes, close, 65535 // self.leads, "65535 (stream, lead) pairs")
        sids, _, lens, ends, n0 = named
        tab = self.rows(_lib.RATE_ROW, named, need_sample=True)
        m0 = np.asarray([self.frontier(v) for v in n0], dtype=np.int64)
        m1 = np.asarray([self.length(v) if e else self.frontier(v) for v, e in zip(n0 + lens, ends)], dtype=np.int64)
        tab["m0"], tab["m"], tab["out_off"] = m0, m1 - m0, np.cumsum(m1 - m0) - (m1 - m0)
        return sids, tab

    def commit(self, tab):
        self.commit_rows(tab, flip=not self.identity)      # the identity keeps no history: its planes never take turns


class ResamplerPool(StreamSurface):
    """Up to `capacity` independent streams of `leads` leads from `fs_in` to `fs_out`, chunk by chunk (`ral_rate_pool`).
    `open()` returns a stream id; `push(chunks, close=())` takes {sid: (leads, c)} (c >= 0, host or device) for any subset of the
    open streams, ends the streams listed in `close`, and returns {sid: (leads, m)} on the device: after n samples a stream has
    been given exactly `rate_frontier(n, up, down)` outputs, and closing it returns the rest.  Concatenated per stream from
    `open` to `close`, the results equal `Resampler.convert(record)` bit for bit, whatever the chunking and the other streams.
    `close(sid, x=None)` ends one stream.  Every argument is checked before any device work (`plan`); a call that raises has
    changed nothing.  A slot keeps its last 2 half / up + 1 samples on the device, in two planes used in turn.  With
    fs_in == fs_out the chunks come back untouched."""

    def __init__(self, fs_in, fs_out, leads, capacity, device="cuda"):
        self.fs_in, self.fs_out = fs_in, fs_out
        up, down = rate_ratio(fs_in, fs_out)
        self.state = RatePoolState(up, down, leads, capacity, type(self).__name__)
        self.up, self.down, self.leads, self.capacity = up, down, self.state.leads, self.state.capacity
        self.identity, self.hist_len = self.state.identity, self.state.hist_len
        self.device = torch.device(device)
        self.bank = self.hist = None
        if not self.identity:
            self.bank = torch.from_numpy(rate_bank(up, down).astype(np.float32)).to(self.device)
            self.hist = torch.zeros(2, self.capacity, self.leads, self.hist_len, dtype=torch.float32, device=self.device)

    def plan(self, shapes, close=()):
        return self.state.plan(shapes, close)

    def commit(self, tab):
        self.state.commit(tab)

    @torch.no_grad()
    def push(self, chunks, close=()):
        xs = as_chunks(chunks)
        sids, tab = self.state.plan({sid: tuple(x.shape) for sid, x in xs.items()}, tuple(close))
        return self.run(xs, sids, tab)

    def run(self, xs, sids, tab):
        """carry out a planned call: xs {sid: chunk tensor} as planned -> {sid: (leads, m)}; commits the plan"""
        dev, leads = self.device, self.leads
        if self.identity:
            self.state.commit(tab)
            empty = torch.empty(leads, 0, dtype=torch.float32, device=dev)
            return {sid: xs[sid].to(device=dev, dtype=torch.float32) if sid in xs else empty for sid in sids}
        out_total = int(tab["m"].sum())
        with torch.cuda.device(dev):
            xp, x_total, _ = pack_chunks(xs, leads, dev)
            out = torch.empty(max(out_total, 1) * leads, dtype=torch.float32, device=dev)
            tab_dev = table_buffer(tab, dev)
            _lib.check(_lib.lib().ral_rate_pool(_ptr(self.hist), _ptr(xp), x_total, tab.ctypes.data, len(tab), _ptr(tab_dev), 1,
                                                self.capacity, leads, self.up, self.down, _ptr(self.bank), self.bank.numel(),
                                                self.hist_len, _ptr(out), out_total, _stream()))
        self.state.commit(tab)
        parts = out[:out_total * leads].split([int(v) * leads for v in tab["m"]])
        return {sid: p.view(leads, -1) for sid, p in zip(sids, parts)}


class RateStreamingDenoiser:
    """`StreamingDenoiser` for records sampled at `fs` instead of the model's `fs_model`: convert to the model's rate
    (`Resampler`), `StreamingDenoiser(model, **kw).denoise`, convert back, keep the first T samples (the round trip gives
    ceil(ceil(T u / d) d / u) >= T).  `denoise(records)` takes (leads, T) or (R, leads, T) at `fs` and returns the same shape at
    `fs`; a record whose converted length is below the model's L is refused on the host.  Works for the 1- and 2-lead models and
    for a 12-lead `NewRALE`.  With fs == fs_model it is `StreamingDenoiser.denoise`."""

    def __init__(self, model, fs, fs_model=MODEL_RATE, **kw):
        self.stream = StreamingDenoiser(model, **kw)
        self.model, self.L, self.leads = model, self.stream.L, self.stream.leads
        dev = self.stream.eng.device
        self.fs, self.fs_model = fs, fs_model
        self.to_model, self.back = Resampler(fs, fs_model, dev), Resampler(fs_model, fs, dev)
        self.window = self.back.length(self.L)       # a model window, in samples at fs

    def _records(self, records, what):
        rec = torch.as_tensor(records)
        if rec.dim() not in (2, 3) or rec.shape[-2] != self.leads:
            raise _lib.RalError(f"{what}: expected a record of shape ({self.leads}, T) or (R, {self.leads}, T), got "
                                f"{tuple(rec.shape)}")
        T = rec.shape[-1]
        if self.to_model.length(T) < self.L:
            raise _lib.RalError(f"{what}: a record of {T} samples is {self.to_model.length(T)} samples at the model's rate, "
                                f"shorter than one window ({self.L})")
        return rec, T

    @torch.no_grad()
    def denoise(self, records):
        rec, T = self._records(records, "RateStreamingDenoiser.denoise")
        if self.to_model.identity:
            return self.stream.denoise(rec)
        y = self.stream.denoise(self.to_model.convert(rec), copy=False)
        return self.back.convert(y)[..., :T].contiguous()

    def evaluate(self, records, noise, snr_db, offsets=None, rng=None, window=None):
        """`StreamingDenoiser.evaluate` at `fs`: `mix_records` (z-score + noise at `snr_db`) on the records as they are,
        `denoise`, `score_records` against the clean records at `fs`; tiles of `window` samples (default: the length of a model
        window at `fs`)."""
        from .evaluate import mix_records, score_records
        if not torch.is_tensor(records) or records.dim() != 3 or records.shape[1] != self.leads:
            raise _lib.RalError(f"evaluate: expected a device tensor of records of shape (R, {self.leads}, T)")
        self._records(records, "RateStreamingDenoiser.evaluate")
        noisy, clean = mix_records(records, noise, snr_db, offsets, rng)
        return score_records(clean, self.denoise(noisy), noisy, self.window if window is None else window)


class RateLivePool(StreamSurface):
    """`LivePool` for streams sampled at `fs`: the same surface (`open`, `push`, `close`, `samples_in`, `open_streams`) with
    chunks at `fs` in and samples at `fs` out.  Three pools in a chain: `ResamplerPool` (fs -> fs_model), `LivePool` or
    `NewRALELivePool` by the model's type, `ResamplerPool` (fs_model -> fs).  Concatenated per stream from `open` to `close`, the
    results equal `RateStreamingDenoiser(model, fs, overlap=overlap).denoise(record)` bit for bit and have exactly T samples.
    All three stages are planned on the host before the first launch (their lengths follow from the counters alone), so a call
    that raises - closing a stream whose length at the model's rate is below L among them - has changed nothing.  A stream whose
    chunk converts to no sample at the model's rate is left out of the inner call."""

    def __init__(self, model, fs, capacity, overlap=0, fs_model=MODEL_RATE):
        adapter = isinstance(model, NewRALE)
        self.inner = (NewRALELivePool if adapter else LivePool)(model, capacity, overlap)
        self.model, self.leads, self.L, self.capacity = model, self.inner.leads, self.inner.L, self.inner.capacity
        dev = self.inner.eng.device
        self.fs, self.fs_model = fs, fs_model
        self.front = ResamplerPool(fs, fs_model, self.leads, capacity, dev)
        self.back = ResamplerPool(fs_model, fs, self.leads, capacity, dev)
        self.front.state.name = self.back.state.name = type(self).__name__
        self.ids = {}        # sid (that of the front pool) -> (inner sid, back sid, samples given so far)

    open_streams = property(lambda self: self.front.open_streams)

    def open(self):
        """-> the sid of a new stream; RalError when `capacity` streams are open"""
        sid = self.front.open()
        self.ids[sid] = [self.inner.open(), self.back.open(), 0]
        return sid

    def samples_in(self, sid):
        return self.front.samples_in(sid)

    @torch.no_grad()
    def push(self, chunks, close=()):
        """chunks {sid: (leads, c) samples at fs, host or device}, close: the sids that end with this call -> {sid: the samples
        at fs that became final, (leads, m) on the device} for every sid named"""
        name = type(self).__name__
        self.inner._ready("push")
        xs = as_chunks(chunks)
        close = tuple(close)
        for sid, x in xs.items():
            if x.dim() == 2 and x.shape[1] == 0 and sid not in close:
                raise _lib.RalError(f"{name}.push: stream {sid}: an empty chunk (only a closing stream may come without samples)")
        # plan the three stages; nothing changes before all three stand
        sids, tab1 = self.front.state.plan({sid: tuple(x.shape) for sid, x in xs.items()}, close)
        ends = {sid: not (f & _lib.POOL_KEEP) for sid, f in zip(sids, tab1["flags"])}
        m1 = {sid: int(m) for sid, m in zip(sids, tab1["m"])}
        mid = [sid for sid in sids if m1[sid] or ends[sid]]          # the streams the inner pool sees in this call
        m2 = {sid: 0 for sid in sids}
        if mid:
            isid = {sid: self.ids[sid][0] for sid in mid}
            try:
                _, tab2, _ = self.inner.state.plan({isid[sid]: (self.leads, m1[sid]) for sid in mid if m1[sid]},
                                                   tuple(isid[sid] for sid in mid if ends[sid]))
            except _lib.RalError as e:
                raise _lib.RalError(f"{name}.push: at the model's rate ({self.fs_model} Hz; streams {isid} there): {e}") from None
            by_slot = {int(s): int(m) for s, m in zip(tab2["slot"], tab2["m"])}
            m2.update({sid: by_slot[isid[sid]] for sid in mid})
        bsid = {sid: self.ids[sid][1] for sid in sids}
        self.back.state.plan({bsid[sid]: (self.leads, m2[sid]) for sid in sids}, tuple(bsid[sid] for sid in sids if ends[sid]))
        # run them
        y1 = self.front.run(xs, sids, tab1)
        y2 = {}
        if mid:
            y2 = self.inner.push({isid[sid]: y1[sid] for sid in mid if m1[sid]}, tuple(isid[sid] for sid in mid if ends[sid]))
        empty = torch.empty(self.leads, 0, dtype=torch.float32, device=self.front.device)
        y3 = self.back.push({bsid[sid]: y2.get(self.ids[sid][0], empty) for sid in sids},
                            tuple(bsid[sid] for sid in sids if ends[sid]))
        out = {}
        for sid, n1 in zip(sids, tab1["n0"] + tab1["c"]):
            y = y3[bsid[sid]]
            if ends[sid]:          # the round trip gives ceil(ceil(T u / d) d / u) >= T samples: keep T
                y = y[:, :int(n1) - self.ids[sid][2]]
                del self.ids[sid]
            else:
                self.ids[sid][2] += y.shape[1]
            out[sid] = y
        return out
