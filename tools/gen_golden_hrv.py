"""Writes tests/golden/g11_hrv.npz: three beat lists of 120 s at 360 Hz with V and S beats (`synth.make_beats_with_hrv`, seed 11)
and what the fp64 restatement `hrv_util.oracle_record` gives for their windows of 30 s every 10 s with min_nn = 8.  numpy only
(written with the version the file records).  The file pins the RESTATEMENT of the definition in include/ralenet.h.

    python tools/gen_golden_hrv.py

pos, lab  int32 (3, cap), padded with -1   n  int64 (3,)   T, win_s, hop_s, min_nn   and per window, record by record:
counts  int64 (N, 4)   stats  fp64 (N, 10)   psd  fp64 (N, F)   S  fp64 (N,)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hrv_util as U  # noqa: E402
from ecg_denoise_amd import hrv_geometry, synth  # noqa: E402

T, WIN_S, HOP_S, MIN_NN = 43200, 30, 10, 8


def main():
    beats, labels = synth.make_beats_with_hrv(3, T, seed=11, p_v=0.06, p_s=0.06)
    g = hrv_geometry(360, WIN_S, HOP_S, min_nn=MIN_NN)
    cap = max(len(b) for b in beats)
    pos, lab = np.full((3, cap), -1, dtype=np.int32), np.full((3, cap), -1, dtype=np.int32)
    for r in range(3):
        pos[r, :len(beats[r])], lab[r, :len(beats[r])] = beats[r], labels[r]
    rows = [o for r in range(3) for o in U.oracle_record(beats[r], labels[r], T, g)]
    out = {"numpy_version": np.array(np.__version__), "pos": pos, "lab": lab, "n": np.array([len(b) for b in beats]),
           "T": np.array(T), "win_s": np.array(WIN_S), "hop_s": np.array(HOP_S), "min_nn": np.array(MIN_NN),
           "counts": np.array([o["counts"] for o in rows], dtype=np.int64), "stats": np.array([o["stats"] for o in rows]),
           "psd": np.array([o["psd"] for o in rows]), "S": np.array([o["S"] for o in rows])}
    assert {1, 2} <= set(lab.reshape(-1).tolist()) and np.isfinite(out["stats"][:, 5:9]).all()
    path = os.path.join(ROOT, "tests", "golden", "g11_hrv.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(rows), "windows")
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
