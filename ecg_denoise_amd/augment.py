"""Training batches mixed on the device (`ral_mix_batch`): the step in front of the training loop.

The reference mixes its windows once, on disk, at one noise kind and one SNR per file (local_utils/local_utils.py:176-192,
261-266; data_utils.py:88-117), so one model is trained per cell of the {bw, ma, em, emb} x {-4 .. 4 dB} grid and every epoch
sees the same noise segment on the same window.  `NoiseMixSampler` keeps the clean rows and the noise records on the device and
draws, for every window of every batch, the clean row and its crop, the noise kind, the noise segment and the SNR, z-scores and
mixes - one kernel launch per batch, nothing from the host on the path:

    sampler = NoiseMixSampler(clean, {"bw": bw, "ma": ma, "em": em}, L=512, snr_db=(-4.0, 4.0))
    train(1, model, 2048, sampler.loader(2048, 500), sampler.loader(2048, 20, replay=True), ...)

A sample is a pure function of (seed, ordinal): the sequence is reproducible, resumable from `state_dict()`, and `world` ranks
drawing their shards get exactly the batch one process would have drawn.  No CPU fallback."""
import ctypes as C
import math

import torch

from . import _lib
from .model import _ptr, _stream

MAX_KINDS = 8


def kind_thresholds(weights):
    """the K uint32 thresholds of the kind draw: floor(2^32 * cumulative share) of non-negative weights (kind = the first k with
    A[2] < cum[k]); the last kind takes the rest, so its threshold is 2^32 - 1 and never read.  A zero weight repeats its
    predecessor's threshold: that kind is never drawn (a trailing zero weight keeps the 2^-32 a uint32 threshold cannot
    express - leave such a kind out instead)."""
    w = [float(x) for x in weights]
    if not 1 <= len(w) <= MAX_KINDS:
        raise _lib.RalError(f"need 1 to {MAX_KINDS} noise kinds; got {len(w)}")
    total = math.fsum(w)
    if not all(math.isfinite(x) and x >= 0.0 for x in w) or not total > 0.0:
        raise _lib.RalError(f"weights must be finite, non-negative and not all zero; got {w}")
    cum, acc = [], 0.0
    for x in w[:-1]:
        acc += x
        cum.append(min(int(math.floor(4294967296.0 * (acc / total))), 0xFFFFFFFF))
    return cum + [0xFFFFFFFF]


class MixedBatch:
    """What `NoiseMixSampler.batch` returns, all device tensors: `noisy`, `clean` (B, leads, L) fp32; the draws `row`, `start`,
    `kind` (an index into the sampler's `.kinds`), `offset` (B,) and `snr_db` (B,) fp64."""
    __slots__ = ("noisy", "clean", "row", "start", "kind", "offset", "snr_db", "first")

    def __init__(self, noisy, clean, row, start, kind, offset, snr_db, first):
        self.noisy, self.clean, self.row, self.start, self.kind, self.offset = noisy, clean, row, start, kind, offset
        self.snr_db, self.first = snr_db, first


class _MixLoader:
    """`steps` batches of (noisy, clean) device tensors per iteration; what `train()` takes for either loader argument"""

    def __init__(self, sampler, batch_size, steps, start):
        self.sampler, self.batch_size, self.steps, self.start = sampler, int(batch_size), int(steps), start

    def __len__(self):
        return self.steps

    def __iter__(self):
        s = self.sampler
        for i in range(self.steps):
            if self.start is None:
                b = s.batch(self.batch_size)
            else:
                b = s._mix(s._rank_first(self.start + i * s.world * self.batch_size, self.batch_size), self.batch_size, None)
            yield b.noisy, b.clean


class NoiseMixSampler:
    """clean (N, leads, Lsrc) and noises - a dict name -> (leads, Tn) or a (K, leads, Tn) stack - arrays or tensors, uploaded once
    (at the first batch).  Every window is the z-scored crop [start, start + L) of a drawn clean row plus the segment
    [offset, offset + L) of a drawn noise kind, scaled to an SNR drawn uniformly in snr_db = [lo, hi) dB; `weights` are the kinds'
    shares (equal when None).  `L` defaults to Lsrc (a window bank: no crop).

    The sequence is counted in ordinals: `batch(B)` on rank r of `world` takes [position + r B, position + (r + 1) B) and
    advances `position` by world * B, on every rank alike."""

    def __init__(self, clean, noises, L=None, snr_db=(-4.0, 4.0), weights=None, seed=2023, rank=0, world=1, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.RalError("NoiseMixSampler mixes on the GPU: give it a HIP device (there is no CPU fallback)")
        if isinstance(noises, dict):
            self.kinds = tuple(noises)
            recs = [noises[k] for k in self.kinds]
        else:
            recs = list(noises)
            self.kinds = tuple(f"noise{k}" for k in range(len(recs)))
        shapes = [tuple(r.shape) for r in recs]
        if not recs or any(len(s) != 2 for s in shapes):
            raise _lib.RalError(f"noises must be a dict name -> (leads, Tn) or a (K, leads, Tn) stack; got shapes {shapes}")
        if len(set(shapes)) != 1:
            raise _lib.RalError("the noise records must have one shape (leads, Tn): crop them to the shortest; got "
                                + ", ".join(f"{k}: {s}" for k, s in zip(self.kinds, shapes)))
        if len(clean.shape) != 3 or clean.shape[1] != shapes[0][0]:
            raise _lib.RalError(f"clean must be (N, leads, Lsrc) with the noise records' {shapes[0][0]} leads; got "
                                f"{tuple(clean.shape)}")
        self.N, self.leads, self.Lsrc = (int(v) for v in clean.shape)
        self.K, self.Tn = len(recs), int(shapes[0][1])
        self.L = self.Lsrc if L is None else int(L)
        self.snr_db = (float(snr_db[0]), float(snr_db[1]))
        self.thresholds = kind_thresholds([1.0] * self.K if weights is None else
                                          [weights[k] for k in self.kinds] if isinstance(weights, dict) else weights)
        if len(self.thresholds) != self.K:
            raise _lib.RalError(f"{len(self.thresholds)} weights for {self.K} noise kinds")
        self.seed, self.rank, self.world = int(seed) & (2 ** 64 - 1), int(rank), int(world)
        if not 0 <= self.rank < self.world:
            raise _lib.RalError(f"need 0 <= rank < world; got rank={rank} world={world}")
        self.position = 0
        self._cum = (C.c_uint32 * self.K)(*self.thresholds)
        self._host = (clean, recs)        # until the first batch
        self._bank = self._noise = None
        # the geometry against the library's rules now, not at the first batch (no device call: ral_mix_draw runs on the host)
        self.draw(0)

    # ---- the sequence (host side)
    def _rank_first(self, position, B):
        return (position + self.rank * B) & (2 ** 64 - 1)

    def advance(self, B):
        """-> the first ordinal of this rank's next `B` samples; moves `position` past the `world * B` of all ranks"""
        B = int(B)
        if B < 1:
            raise _lib.RalError(f"need B >= 1; got {B}")
        first = self._rank_first(self.position, B)
        self.position = (self.position + self.world * B) & (2 ** 64 - 1)
        return first

    def draw(self, ordinal):
        """(row, start, kind, offset, snr_db) of one ordinal, computed on the host by the code the kernel runs"""
        d, snr = (C.c_int32 * 4)(), C.c_double()
        _lib.check(_lib.lib().ral_mix_draw(self.N, self.Lsrc, self.L, self.K, self.Tn, self._cum, self.snr_db[0], self.snr_db[1],
                                           self.seed, int(ordinal) & (2 ** 64 - 1), d, C.byref(snr)))
        return d[0], d[1] & 0xFFFFFFFF, d[2], d[3] & 0xFFFFFFFF, snr.value

    def _config(self):
        return {"N": self.N, "leads": self.leads, "Lsrc": self.Lsrc, "L": self.L, "Tn": self.Tn, "kinds": list(self.kinds),
                "thresholds": list(self.thresholds), "snr_db": list(self.snr_db)}

    def state_dict(self):
        """seed, position and configuration: plain host values"""
        return {"seed": self.seed, "position": self.position, "world": self.world, "config": self._config()}

    def load_state_dict(self, state):
        """continue the sequence of a saved sampler; its configuration must be this one's (the data itself is not compared)"""
        if state["config"] != self._config():
            diff = {k: (v, self._config().get(k)) for k, v in state["config"].items() if self._config().get(k) != v}
            raise _lib.RalError(f"the saved sampler was configured differently (saved, this one): {diff}")
        self.seed, self.position = int(state["seed"]), int(state["position"])

    # ---- the device side
    def _upload(self):
        clean, recs = self._host
        f32 = lambda a: torch.as_tensor(a).to(device=self.device, dtype=torch.float32)
        self._bank = f32(clean).contiguous()
        self._noise = torch.stack([f32(r) for r in recs]).contiguous()
        self._host = None

    def _mix(self, first, B, rows):
        if self._bank is None:
            self._upload()
        dev = self.device
        if rows is not None:
            if not torch.is_tensor(rows) or tuple(rows.shape) != (B,):
                raise _lib.RalError(f"rows must be a tensor of {B} row indices")
            rows = rows.to(device=dev, dtype=torch.int64).contiguous()
        with torch.cuda.device(dev):
            noisy = torch.empty(B, self.leads, self.L, dtype=torch.float32, device=dev)
            clean = torch.empty_like(noisy)
            draws = torch.empty(B, 4, dtype=torch.int32, device=dev)
            snr = torch.empty(B, dtype=torch.float64, device=dev)
            _lib.check(_lib.lib().ral_mix_batch(_ptr(self._bank), _ptr(self._noise), _ptr(rows), self.N, self.leads, self.Lsrc,
                                                self.L, self.K, self.Tn, self._cum, self.snr_db[0], self.snr_db[1], self.seed,
                                                first, B, _ptr(noisy), _ptr(clean), _ptr(draws), _ptr(snr), _stream()))
        # start and offset are unsigned 32-bit columns: widen them where the range does not fit int32
        col = lambda j, span: draws[:, j] if span <= 2 ** 31 else draws[:, j].to(torch.int64) & 0xFFFFFFFF
        return MixedBatch(noisy, clean, draws[:, 0], col(1, self.Lsrc - self.L + 1), draws[:, 2], col(3, self.Tn - self.L + 1),
                          snr, first)

    def batch(self, B, rows=None):
        """this rank's next `B` windows -> `MixedBatch`.  `rows` (B,) int64 device tensor: the clean rows to use instead of the
        drawn ones (a slice of a device permutation: sampling without replacement); every other field is drawn as without it."""
        return self._mix(self.advance(B), int(B), rows)

    def loader(self, batch_size, steps, replay=False):
        """an iterable of `steps` (noisy, clean) batches, as `train()` takes them.  replay=False: every iteration continues the
        sequence.  replay=True: a fixed set - `steps * world * batch_size` ordinals are set aside now (the sequence moves past
        them) and every iteration yields exactly those."""
        start = None
        if replay:
            start = self.position
            for _ in range(int(steps)):
                self.advance(batch_size)
        return _MixLoader(self, batch_size, steps, start)
