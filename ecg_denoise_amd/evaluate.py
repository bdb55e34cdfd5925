"""Noise-stress evaluation of streamed denoising, on the device (the second half of the project's metric, SNR
improvement in dB, for whole records through the path that is deployed).

The reference's experiment grid (run.sh: models x {bw, ma, em, emb} x {-4 .. 4 dB}, one `snr:..., rmse:...` line each) mixes noise
into 256-sample windows on the host (local_utils/local_utils.py:86-130) and scores them in torch (local_utils/evaluate.py:10-51,
denoise_train.py:82-89).  Here the same rule runs on record groups (R, leads, T) of any length:

    noisy, clean = mix_records(records, noise, snr_db)            # ral_mix_records: z-score + SNR-scaled noise segment
    out = StreamingDenoiser(model, ...).denoise(noisy)
    scores = score_records(clean, out, noisy, window=model L)     # ral_score_records: SNR / RMSE in and out

or `StreamingDenoiser.evaluate(records, noise, snr_db)` for the three at once.  One call covers a whole intensity sweep: `snr_db`
may differ from record to record.  No CPU fallback."""
import random

import numpy as np
import torch

from . import _lib
from .model import _ptr, _stream
from .pools import scratch_bytes

COLUMNS = ("snr_in_db", "snr_out_db", "rmse_in", "rmse_out")


def draw_offsets(R, T, Tn, rng=None):
    """the noise offset of each of R records as the reference draws it (`random.randint(0, len(noise) - len - 1)`,
    local_utils/local_utils.py:124): one `rng.randint(0, Tn - T - 1)` per record, in record order, from a `random.Random`;
    0 without a draw when Tn - T < 1"""
    rng = rng or random.Random()
    return [rng.randint(0, Tn - T - 1) if Tn - T >= 1 else 0 for _ in range(R)]


def mix_records(records, noise, snr_db, offsets=None, rng=None):
    """records (R, leads, T) and noise (leads, Tn), device tensors (any float/int dtype), Tn >= T -> fp32 (noisy, clean), each
    (R, leads, T): `clean[r]` is the per-lead z-score of the record over its whole length (`np_norm`), `noisy[r]` adds
    noise[:, offsets[r] : offsets[r] + T] scaled to `snr_db[r]` dB (`Gnoisegen`) - the rule of `data.prep_windows` per record.
    `snr_db`: a scalar or one value per record; `offsets`: one per record, drawn by `draw_offsets(R, T, Tn, rng)` when not
    given.  A constant lead is not floored (as in `prep_windows`)."""
    if not (torch.is_tensor(records) and torch.is_tensor(noise) and records.is_cuda and noise.is_cuda):
        raise _lib.RalError("mix_records runs on the GPU: pass device tensors (there is no CPU fallback)")
    if records.dim() != 3 or noise.dim() != 2 or noise.shape[0] != records.shape[1]:
        raise _lib.RalError(f"records must be (R, leads, T) and noise (leads, Tn); got {tuple(records.shape)} and "
                            f"{tuple(noise.shape)}")
    rec = records.to(torch.float32).contiguous()
    noi = noise.to(device=rec.device, dtype=torch.float32).contiguous()
    R, leads, T = rec.shape
    Tn = noi.shape[1]
    snr = np.ascontiguousarray(np.broadcast_to(np.asarray(snr_db, dtype=np.float64), (R,)) if np.ndim(snr_db) == 0
                               else np.asarray(snr_db, dtype=np.float64))
    off = np.asarray(draw_offsets(R, T, Tn, rng) if offsets is None else offsets, dtype=np.int64)
    if snr.shape != (R,) or off.shape != (R,):
        raise _lib.RalError(f"snr_db must be a scalar or {R} values and offsets {R} values (one per record)")
    lib = _lib.lib()
    nbytes = scratch_bytes(lib.ral_mix_records_scratch_bytes(R, leads, T))
    with torch.cuda.device(rec.device):
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=rec.device)
        noisy, clean = torch.empty_like(rec), torch.empty_like(rec)
        _lib.check(lib.ral_mix_records(_ptr(rec), _ptr(noi), R, leads, T, Tn, off.ctypes.data, snr.ctypes.data, _ptr(scratch),
                                       _ptr(noisy), _ptr(clean), _stream()))
    return noisy, clean


def stress_front(denoiser, records, noise, snr_db, offsets=None, rng=None):
    """the front of every noise-stress evaluation of a downstream statistic (`evaluate_beats`, `evaluate_rhythm`,
    `evaluate_intervals`, `evaluate_hrv`, `evaluate_templates`, `evaluate_pst`): `mix_records(records, noise, snr_db, offsets, rng)`, then `denoiser.denoise(noisy)` ->
    (fs, device, clean, noisy, denoised); `fs` is the denoiser's outer rate, 360 Hz where it names none, `device` that of the
    records, where the caller's default detector, classifier and so on belong"""
    noisy, clean = mix_records(records, noise, snr_db, offsets, rng)            # (refuses anything but device tensors)
    return getattr(denoiser, "fs", 360), records.device, clean, noisy, denoiser.denoise(noisy)


class RecordScores:
    """What `score_records` returns: four fp64 device tensors whose last axis is (snr_in_db, snr_out_db, rmse_in, rmse_out) -
    `per_lead` (R, leads, 4), `per_record` (R, 4), `per_window` (R, nwin, 4) and `window_mean` (R + 1, 4), whose last row is the
    mean over all tiles of all records (the number the reference's `output.txt` holds).  Without `noisy` the "in" columns are
    NaN.  Zero error is +inf dB."""

    def __init__(self, per_lead, per_record, per_window, window_mean, window):
        self.per_lead, self.per_record, self.per_window, self.window_mean = per_lead, per_record, per_window, window_mean
        self.window = int(window)

    @property
    def snr_imp_db(self):
        """SNR improvement, snr_out_db - snr_in_db, of each of the four tensors (same leading shape)"""
        return {k: getattr(self, k)[..., 1] - getattr(self, k)[..., 0]
                for k in ("per_lead", "per_record", "per_window", "window_mean")}

    def summary(self):
        """plain floats of the all-tiles row (synchronises)"""
        row = self.window_mean[-1].tolist()
        d = dict(zip(COLUMNS, row))
        d["snr_imp_db"] = row[1] - row[0]
        return d

    def output_line(self, model_name, epoch, noise_name, intensity):
        """the line the reference appends to output.txt per run (denoise_train.py:101; `train.train` here)"""
        s = self.summary()
        return f"{model_name}_{epoch}_{noise_name}_intensity{intensity}:snr:{s['snr_out_db']}, rmse:{s['rmse_out']}\n"


def score_records(clean, out, noisy=None, window=256):
    """clean, out and optionally noisy, device tensors (R, leads, T) -> `RecordScores`: SNR and RMSE of `out` (and of `noisy`)
    against `clean` per lead, per record, per tile of `window` samples x all leads, and the tile means; double sums,
    bit-reproducible.  1 <= window <= T; a trailing partial tile counts per lead and per record only."""
    ts = [clean, out] + ([noisy] if noisy is not None else [])
    if not all(torch.is_tensor(t) and t.is_cuda for t in ts):
        raise _lib.RalError("score_records runs on the GPU: pass device tensors (there is no CPU fallback)")
    if clean.dim() != 3 or any(t.shape != clean.shape or t.device != clean.device for t in ts):
        raise _lib.RalError("clean, out and noisy must be (R, leads, T) tensors of one shape on one device; got "
                            + ", ".join(str(tuple(t.shape)) for t in ts))
    c, o = (t.to(torch.float32).contiguous() for t in ts[:2])
    n = noisy.to(torch.float32).contiguous() if noisy is not None else None
    R, leads, T = c.shape
    W = int(window)
    lib = _lib.lib()
    nbytes = scratch_bytes(lib.ral_score_records_scratch_bytes(R, leads, T, W))
    with torch.cuda.device(c.device):
        e = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=c.device)
        scratch = e(nbytes // 8)
        sc = RecordScores(e(R, leads, 4), e(R, 4), e(R, T // W, 4), e(R + 1, 4), W)
        _lib.check(lib.ral_score_records(_ptr(c), _ptr(o), _ptr(n), R, leads, T, W, _ptr(scratch), _ptr(sc.per_lead),
                                         _ptr(sc.per_record), _ptr(sc.per_window), _ptr(sc.window_mean), _stream()))
    return sc
