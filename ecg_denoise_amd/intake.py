"""Where the arguments of beat analysis enter, for the detector, the classifier, the delineator, the HRV analyser and
`match_beats`: the record argument in two steps (`record_shape`, `device_records`), so that a call is refused for its shape,
then its geometry, then its beat lists, and only then for not being on a device; `Beats` and `beat_lists`, the one way a beat
list becomes padded device tensors; `pad_rows`; `check_leads`.  A leaf: of the package it imports `_lib` alone.  Every message
begins with the caller's name, which the caller passes."""
import numbers
from fractions import Fraction

import numpy as np
import torch

from . import _lib


def check_leads(leads, what, most=None):
    """raise RalError unless `leads` is an int >= 1 (and <= `most`); `what` names the analysis in the message"""
    if isinstance(leads, bool) or not isinstance(leads, numbers.Integral) or leads < 1 or (most is not None and leads > most):
        rule = ">= 1" if most is None else f"in [1, {most}]"
        raise _lib.RalError(f"{what}: leads must be {rule} (got {leads!r})")


def record_shape(records, what):
    """step one, on the host: `records` must be a tensor (leads, T) or (R, leads, T) with no empty axis -> (R, leads, T)"""
    if not torch.is_tensor(records):
        raise _lib.RalError(f"{what} runs on the GPU: pass a device tensor (there is no CPU fallback)")
    if records.dim() not in (2, 3) or records.shape[-1] < 1 or records.shape[-2] < 1 or records.shape[0] < 1:
        raise _lib.RalError(f"{what}: expected (leads, T) or (R, leads, T) with T >= 1, got {tuple(records.shape)}")
    return (1,) + tuple(records.shape) if records.dim() == 2 else tuple(records.shape)


def device_records(records, what):
    """step two, after every host check: a host tensor is refused -> the records as a contiguous fp32 device tensor"""
    if not records.is_cuda:
        raise _lib.RalError(f"{what} runs on the GPU: pass a device tensor (there is no CPU fallback)")
    return records.to(torch.float32).contiguous()


class Beats:
    """What `BeatDetector.detect` returns: `peaks` (R, cap) int32, each row the record's R-peak sample indices in ascending
    order padded with -1, and `count` (R,) int32, both on the device; `fs` is the rate the indices refer to."""

    def __init__(self, peaks, count, fs=360):
        self.peaks, self.count, self.fs = peaks, count, fs

    def __len__(self):
        return self.peaks.shape[0]

    def tolist(self):
        """-> [[peak indices of record r] for r] as plain ints (synchronises)"""
        return [row[:n] for row, n in zip(self.peaks.tolist(), self.count.tolist())]

    def rr_seconds(self):
        """-> per record the RR intervals in seconds, a float64 numpy array of count - 1 values (synchronises)"""
        fs = float(Fraction(self.fs))
        return [np.diff(np.asarray(p, dtype=np.float64)) / fs for p in self.tolist()]


def pad_rows(rows, fill, dtype=np.int32, shape=None):
    """rows of unequal length -> an array of `dtype`, row i holding rows[i] and then `fill`; (len(rows), max(1, the longest
    row)) unless `shape` names a larger one"""
    pad = np.full(shape or (len(rows), max(1, max(len(r) for r in rows))), fill, dtype=dtype)
    for i, r in enumerate(rows):
        pad[i, :len(r)] = r
    return pad


def beat_lists(beats, device, what, T=None, strict=True, R=None, name=None):
    """`Beats`, or one list (or tensor) of ascending sample indices per record -> ((R, cap) int32 padded with -1, (R,) int32)
    on `device`.  The indices lie in [0, T), without T in [0, 2^31), and ascend strictly or, without `strict`, may repeat.  R is
    the number of records the caller has: so many lists, and a `Beats` must hold R records on `device`; without R at least one
    list, and a `Beats` is trusted (there is nothing to hold it against).  `what`, the caller's name, begins every message;
    `name` is what the caller calls this argument, if it takes two lists."""
    if isinstance(beats, Beats):
        if R is not None and (beats.peaks.shape[0] != R or beats.peaks.device != device):
            raise _lib.RalError(f"{what}: {beats.peaks.shape[0]} beat lists on {beats.peaks.device} for {R} "
                                f"records on {device}")
        return beats.peaks.contiguous(), beats.count.contiguous()
    rows = [np.asarray(r.cpu() if torch.is_tensor(r) else r, dtype=np.int64).reshape(-1) for r in beats]
    if R is not None and len(rows) != R:
        raise _lib.RalError(f"{what}: {len(rows)} beat lists for {R} records")
    if not rows:
        raise _lib.RalError(f"{what}: {name} holds no record" if name else f"{what}: no record")
    end = 2 ** 31 if T is None else T
    for r in rows:
        if len(r) and (r[0] < 0 or r[-1] >= end or np.any(np.diff(r) < (1 if strict else 0))):
            raise _lib.RalError(f"{what}: {name + ' must hold' if name else 'the beats of a record must be'} "
                                f"{'strictly ascending positions' if strict else 'ascending sample indices'} in "
                                f"[0, {'2^31' if T is None else T})")
    return torch.from_numpy(pad_rows(rows, -1)).to(device), torch.tensor([len(r) for r in rows], dtype=torch.int32, device=device)
