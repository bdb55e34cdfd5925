"""What every stream pool shares on the host: up to `capacity` independent streams in slots, pushed chunk by chunk, every call
planned and checked before any device work.

    SlotState      which slots hold an open stream, how many samples each has received, which of its two history planes is
                   current; the argument checks every pool makes (`named`), the columns every table shares (`rows`) and the
                   common commit (`commit_rows`)
    as_chunks      a call's chunks as tensors
    pack_chunks    a call's chunks in one device buffer, row r's (leads, c) at x_off * leads
    table_buffer   the device buffer for a call's table
    scratch_bytes  the size a `ral_*_scratch_bytes` call returned, or the library's last error
    StreamSurface  `open_streams`, `open`, `samples_in`, `close` for a class with a `.state` and a `push`

A pool's own state class derives from `SlotState` and adds its geometry checks, its refusals, its table and what is special in
its commit (`infer.PoolState`, `rate.RatePoolState`, `beats.BeatPoolState`); the pool itself takes `StreamSurface`, plans with
its state, packs with `pack_chunks` and launches.  A further pool starts here."""
import numpy as np
import torch

from . import _lib


class SlotState:
    """The slots of a pool, without a device.  `n[slot]` samples received, `turn[slot]` the current history plane, `is_open[slot]`,
    and `free`, the slots to hand out next (popped from the end: slot 0 first).  A sid is its stream's slot."""

    def __init__(self, capacity, leads, name):
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 1:
            raise _lib.RalError(f"{name}: capacity must be >= 1")
        self.capacity, self.leads, self.name = int(capacity), int(leads), name
        self.n = np.zeros(self.capacity, dtype=np.int64)
        self.turn = np.zeros(self.capacity, dtype=np.int32)
        self.is_open = np.zeros(self.capacity, dtype=bool)
        self.free = list(range(self.capacity - 1, -1, -1))

    def open(self):
        if not self.free:
            raise _lib.RalError(f"{self.name}.open: all {self.capacity} slots hold an open stream")
        sid = self.free.pop()
        self.n[sid], self.is_open[sid] = 0, True
        return sid

    def _is_open(self, sid):
        return isinstance(sid, (int, np.integer)) and not isinstance(sid, bool) and 0 <= sid < self.capacity \
            and bool(self.is_open[sid])

    def _need_open(self, sid, where):
        if not self._is_open(sid):
            raise _lib.RalError(f"{where}: {sid!r} is not an open stream")

    def named(self, shapes, close, max_rows=None, rows_what=None):
        """shapes {sid: shape of its chunk, (leads, c) with c >= 0}, close: the sids that end with this call; at most `max_rows`
        streams may be named (`rows_what` words the limit) -> (sids in row order: those with a chunk, then the others that
        close; slot, lens, ends, n0 per row).  Raises RalError for a bad argument; changes nothing."""
        name = self.name
        sids = list(shapes)
        for sid in close:
            if sid not in sids:
                sids.append(sid)
        if not sids:
            raise _lib.RalError(f"{name}.push: nothing to do (no chunk and no stream to close)")
        for sid in sids:
            self._need_open(sid, f"{name}.push")
        if max_rows is not None and len(sids) > max_rows:
            raise _lib.RalError(f"{name}.push: more than {rows_what} in one call")
        lens = np.zeros(len(sids), dtype=np.int64)
        for r, (sid, shape) in enumerate(shapes.items()):
            if len(shape) != 2 or shape[0] != self.leads:
                raise _lib.RalError(f"{name}.push: stream {sid}: expected a chunk of shape ({self.leads}, samples), got "
                                    f"{tuple(shape)}")
            lens[r] = shape[1]
        if np.any(lens > 0x3fffffff):
            raise _lib.RalError(f"{name}.push: a chunk of more than 2^30 - 1 samples")
        slot = np.asarray(sids, dtype=np.int64)
        ends = np.isin(slot, np.asarray(list(close), dtype=np.int64))
        return sids, slot, lens, ends, self.n[slot]

    def rows(self, dtype, named, need_sample=False):
        """named: what `named` returned -> the call's table of `dtype`, zeroed but for the columns every pool shares: n0, c, x_off
        (the chunks packed in row order), slot, its current turn, and T = n0 + c without POOL_KEEP for a row that ends, T = -1
        with POOL_KEEP for one that stays open.  need_sample: RalError for a stream that would end without a sample."""
        sids, slot, lens, ends, n0 = named
        n1 = n0 + lens
        if need_sample and np.any(ends & (n1 < 1)):
            r = int(np.argmax(ends & (n1 < 1)))
            raise _lib.RalError(f"{self.name}.push: stream {sids[r]} would end without a single sample")
        tab = np.zeros(len(sids), dtype=dtype)
        tab["n0"], tab["T"], tab["slot"], tab["c"], tab["x_off"] = n0, np.where(ends, n1, -1), slot, lens, np.cumsum(lens) - lens
        tab["turn"], tab["flags"] = self.turn[slot], np.where(ends, 0, _lib.POOL_KEEP)
        return tab

    def commit_rows(self, tab, flip=True):
        """apply a planned call: the rows' new sample counts, the other history plane for the rows that stay open (`flip`), the
        slots of the closing rows back to `free`"""
        slot, keep = tab["slot"], (tab["flags"] & _lib.POOL_KEEP) != 0
        self.n[slot] = tab["n0"] + tab["c"]
        if flip:
            self.turn[slot[keep]] ^= 1
        for sid in slot[~keep]:
            self.is_open[sid] = False
            self.free.append(int(sid))


def as_chunks(chunks):
    return {sid: x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float32))
            for sid, x in chunks.items()}


def pack_chunks(xs, leads, device):
    """xs {sid: (leads, c) tensor, host or device, as planned} -> (xp, x_total, views): the chunks in dict order in one fp32
    buffer on `device` of max(x_total, 1) * leads values, the samples per lead they hold, and {sid: its (leads, c) view of xp}.
    Host chunks, or fp32 device chunks, go over in one copy; a mixture is copied chunk by chunk."""
    x_total = sum(x.numel() for x in xs.values()) // leads
    xp = torch.empty(max(x_total, 1) * leads, dtype=torch.float32, device=device)
    flat = [x.reshape(-1) for x in xs.values() if x.numel()]
    if flat:
        if all(not f.is_cuda for f in flat) or all(f.is_cuda and f.dtype == torch.float32 for f in flat):
            xp[:x_total * leads].copy_(flat[0] if len(flat) == 1 else torch.cat(flat), non_blocking=True)
        else:
            o = 0
            for f in flat:
                xp[o:o + f.numel()].copy_(f, non_blocking=True)
                o += f.numel()
    views, o = {}, 0
    for sid, x in xs.items():
        views[sid] = xp[o:o + x.numel()].view(leads, x.numel() // leads)
        o += x.numel()
    return xp, x_total, views


def table_buffer(tab, device):
    """the device buffer a library call uploads the table `tab` into"""
    return torch.empty(len(tab) * tab.itemsize, dtype=torch.uint8, device=device)


def scratch_bytes(nbytes):
    """what a `ral_*_scratch_bytes` call returned -> that size; RalError with the library's own message if it refused (< 0)"""
    if nbytes < 0:
        raise _lib.RalError(_lib.lib().ral_last_error().decode())
    return nbytes


class StreamSurface:
    """The surface of a pool whose `state` is a `SlotState` and whose `push(chunks, close=())` returns {sid: result}."""

    open_streams = property(lambda self: tuple(int(s) for s in np.flatnonzero(self.state.is_open)))

    def open(self):
        """-> the sid of a new stream (a free slot); RalError when `capacity` streams are open"""
        return self.state.open()

    def samples_in(self, sid):
        self.state._need_open(sid, f"{type(self).__name__}.samples_in")
        return int(self.state.n[sid])

    def close(self, sid, x=None):
        """end one stream, with an optional last chunk -> the rest of its results"""
        return self.push({} if x is None else {sid: x}, close=(sid,))[sid]
