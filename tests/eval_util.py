"""TEST INFRASTRUCTURE ONLY -- fp64 restatement of record-level noise mixing and scoring (ral_mix_records / ral_score_records),
built from the pinned oracles alone: `dataprep_oracle.prep_segment` (called with L = T, result [0]) and `ralenet_oracle.snr` /
`rmse`, so it inherits their pins (tests/golden/g7_dataprep.npz, the metric fixtures).  No reference file is read."""
import numpy as np
import torch

import dataprep_oracle as D
import ralenet_oracle as O


def mix_ref(rec, noise, offsets, snr_db):
    """rec (R, leads, T), noise (leads, Tn) arrays -> float32 (noisy, clean), each (R, leads, T): every record through
    `prep_segment` with its own noise segment and SNR, as one window of T samples"""
    rec, noise = np.asarray(rec), np.asarray(noise)
    R, _, T = rec.shape
    noisy, clean = [], []
    for r in range(R):
        seg = noise[:, offsets[r]:offsets[r] + T]
        n, c = D.prep_segment(rec[r].T, seg.T, float(snr_db[r]), T)
        noisy.append(n[0]); clean.append(c[0])
    return np.stack(noisy), np.stack(clean)


def _tiles(a, W):
    """(R, leads, T) -> (R * nwin, leads, W): tile j of record r = samples [j W, (j + 1) W) of all leads"""
    R, leads, T = a.shape
    nwin = T // W
    return a[:, :, :nwin * W].reshape(R, leads, nwin, W).permute(0, 2, 1, 3).reshape(R * nwin, leads, W)


def _cols(c, o, n):
    """windows (B, ...) -> (B, 4) = (snr_in_db, snr_out_db, rmse_in, rmse_out) by the oracle's per-window metrics"""
    nan = torch.full((c.shape[0],), float("nan"), dtype=torch.float64)
    return torch.stack([O.snr(c, n) if n is not None else nan, O.snr(c, o),
                        O.rmse(c, n) if n is not None else nan, O.rmse(c, o)], dim=1)


def score_ref(clean, out, noisy=None, window=256):
    """fp32 arrays / tensors (R, leads, T) -> dict of fp64 numpy arrays per_lead (R, leads, 4), per_record (R, 4),
    per_window (R, nwin, 4), window_mean (R + 1, 4): the fp32 values converted to double, then `ralenet_oracle.snr` / `rmse`
    on the records regrouped as the "windows" each output covers"""
    f = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).double()
    c, o, n = f(clean), f(out), f(noisy)
    R, leads, T = c.shape
    W = int(window)
    lead = lambda a: None if a is None else a.reshape(R * leads, 1, T)
    tile = lambda a: None if a is None else _tiles(a, W)
    pw = _cols(tile(c), tile(o), tile(n)).reshape(R, T // W, 4)
    wm = torch.cat([pw.mean(1), pw.reshape(-1, 4).mean(0, keepdim=True)])
    return {"per_lead": _cols(lead(c), lead(o), lead(n)).reshape(R, leads, 4).numpy(), "per_record": _cols(c, o, n).numpy(),
            "per_window": pw.numpy(), "window_mean": wm.numpy()}
