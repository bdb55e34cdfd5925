"""Non-neural comparison baselines of the reference's result tables.

`wavelet_denoise` mirrors `local_utils/denoisefunc.py:7-33` (same name, same accepted shapes: a 2-D (rows, L) or 3-D
(batch, leads, L) array of records, result of the same shape): db8 decomposition at the maximum level, soft threshold of
every detail band at 0.04 * max(band), reconstruction - as one HIP kernel (`ral_wavelet_denoise`, a record and its
coefficient pyramid in LDS).  The reference works on NumPy arrays on the host; a NumPy array is accepted here too (it is
copied to the device and back), a CUDA tensor stays on the device.  No CPU fallback.

`fft_denoise` mirrors `local_utils/denoisefunc.py:36-66` (the model "fft" of `test_cls.py:240-255`): per item of the first axis
`X = fft(item); X[|X| < threshold * max|X|] = 0; ifft(X).real` - a row of a 2-D array against its own maximum, all leads of an
item of a 3-D array against one - as `ral_fft_denoise` (a mixed-radix FFT of the row in LDS; a direct transform for the lengths
the FFT does not take).  The reference function itself cannot run (it never imports `fft` / `ifft`); its definition is
restated in tests/fft_util.py.

`ClassicalDenoiser` is the record form of both: `.denoise(records)` cuts (R, leads, T) records into the windows a
`StreamingDenoiser` uses at overlap 0 and runs the baseline on them, so it can stand wherever one is passed for its `.denoise`
(`evaluate_beats`, `evaluate_rhythm`, `score_records`)."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def wavelet_denoise(ecg_data, threshold=0.04, device="cuda:0"):
    is_np = isinstance(ecg_data, np.ndarray)
    x = torch.as_tensor(ecg_data)
    if x.dim() not in (2, 3):
        raise ValueError("wavelet_denoise takes a 2-D (rows, L) or 3-D (batch, leads, L) array")   # the reference returns None
    L = x.shape[-1]
    if L % 2 or L > 8192:
        raise ValueError(f"record length must be even and <= 8192, got {L}")
    xd = x.to(device=device if not x.is_cuda else x.device, dtype=torch.float32).contiguous()
    y = torch.empty_like(xd)
    rows = xd.numel() // L if L else 0
    with torch.cuda.device(xd.device):
        _lib.check(_lib.lib().ral_wavelet_denoise(C.c_void_p(xd.data_ptr()), C.c_void_p(y.data_ptr()), rows, L, float(threshold),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    if is_np:
        return y.cpu().numpy().astype(ecg_data.dtype if ecg_data.dtype.kind == "f" else np.float64)
    return y


def _fft_length_check(L):
    """raises ValueError for a record length `ral_fft_denoise` refuses (asked of the library: host arithmetic, no device)"""
    lib = _lib.lib()
    if lib.ral_fft_denoise_scratch_bytes(0, 1, int(L)) < 0:
        raise ValueError(lib.ral_last_error().decode())


def fft_denoise(ecg_datas, threshold=0.04, device="cuda:0", return_kept=False):
    """-> the denoised array, of the input's shape; with `return_kept` also the surviving bins per item of the first axis
    (int32, counted over the full spectra of its rows)"""
    if isinstance(ecg_datas, (list, tuple)):                   # the reference: np.array(list of 1-D arrays)
        rows = [np.asarray(r) for r in ecg_datas]
        if any(r.ndim != 1 for r in rows) or len({r.shape[0] for r in rows}) > 1:
            raise ValueError("fft_denoise takes a list of 1-D arrays of one length")
        ecg_datas = np.stack(rows) if rows else np.zeros((0, 2))
    is_np = isinstance(ecg_datas, np.ndarray)
    x = torch.as_tensor(ecg_datas)
    if x.dim() not in (2, 3):
        raise ValueError("fft_denoise takes a 2-D (rows, L) or 3-D (batch, leads, L) array, or a list of 1-D arrays")
    groups, rpg, L = x.shape[0], (x.shape[1] if x.dim() == 3 else 1), x.shape[-1]
    _fft_length_check(L)
    if rpg < 1:
        raise ValueError("fft_denoise: a 3-D array needs at least one lead")
    if not float(threshold) >= 0.0:
        raise ValueError(f"fft_denoise: the threshold factor must be non-negative (got {threshold!r})")
    xd = x.to(device=device if not x.is_cuda else x.device, dtype=torch.float32).contiguous()
    y = torch.empty_like(xd)
    kept = torch.empty(groups, dtype=torch.int32, device=xd.device)
    lib = _lib.lib()
    nbytes = lib.ral_fft_denoise_scratch_bytes(groups, rpg, L)
    if nbytes < 0:
        raise _lib.RalError(lib.ral_last_error().decode())
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=xd.device)
    with torch.cuda.device(xd.device):
        _lib.check(lib.ral_fft_denoise(C.c_void_p(xd.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(kept.data_ptr()), groups, rpg,
                                       L, float(threshold), C.c_void_p(scratch.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    if is_np:
        y = y.cpu().numpy().astype(ecg_datas.dtype if ecg_datas.dtype.kind == "f" else np.float64)
        kept = kept.cpu().numpy()
    return (y, kept) if return_kept else y


def classical_window_starts(T, L):
    """the window starts of `StreamingDenoiser` at overlap 0: 0, L, 2L, ... and a last window at T - L when T % L != 0"""
    if T < L:
        raise _lib.RalError(f"record shorter than one window ({T} < {L})")
    return [k * L for k in range(T // L)] + ([T - L] if T % L else [])


class ClassicalDenoiser:
    """`kind` "fft" or "wavelet" on windows of L samples.  `.denoise(records)`: (R, leads, T >= L) -> the same shape; the windows
    start at 0, L, 2L, ... plus one at T - L when T % L != 0, of which only the final T % L samples are kept.  One fft group is
    the `leads` rows of one window of one record; wavelet rows are independent.  `threshold`: None = the reference's 0.04."""

    def __init__(self, kind, L, threshold=None, device="cuda"):
        if kind not in ("fft", "wavelet"):
            raise ValueError(f"ClassicalDenoiser: kind must be 'fft' or 'wavelet' (got {kind!r})")
        self.kind, self.L, self.threshold = kind, int(L), 0.04 if threshold is None else float(threshold)
        if kind == "fft":
            _fft_length_check(self.L)
        elif self.L < 2 or self.L % 2 or self.L > 8192:
            raise ValueError(f"record length must be even and <= 8192, got {L}")
        if not self.threshold >= 0.0:
            raise ValueError(f"ClassicalDenoiser: the threshold factor must be non-negative (got {threshold!r})")
        self.device = device

    def window_starts(self, T):
        return classical_window_starts(int(T), self.L)

    def denoise(self, records):
        is_np = isinstance(records, np.ndarray)
        x = torch.as_tensor(records)
        if x.dim() != 3:
            raise ValueError("ClassicalDenoiser.denoise takes (R, leads, T) records")
        R, leads, T = x.shape
        starts, L = self.window_starts(T), self.L
        xd = x.to(device=self.device if not x.is_cuda else x.device, dtype=torch.float32)
        win = torch.stack([xd[..., s:s + L] for s in starts], dim=1)           # (R, windows, leads, L)
        if self.kind == "fft":
            out = fft_denoise(win.reshape(-1, leads, L), self.threshold)
        else:
            out = wavelet_denoise(win.reshape(-1, L), self.threshold)
        out = out.reshape(R, len(starts), leads, L)
        y = torch.empty_like(xd)
        for i, s in enumerate(starts):                     # (the last window overlaps its neighbour: written last, its tail wins)
            if T % L and i == len(starts) - 1:
                y[..., T - T % L:] = out[:, i, :, L - T % L:]
            else:
                y[..., s:s + L] = out[:, i]
        if is_np:
            return y.cpu().numpy().astype(records.dtype if records.dtype.kind == "f" else np.float64)
        return y
