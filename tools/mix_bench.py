"""What feeding the training loop costs on one MI355X: `NoiseMixSampler` (ral_mix_batch: windows drawn and mixed on the device)
against the host loader (`make_loaders`: NumPy fancy indexing per batch, uploaded from pageable memory by `train()`).

  1. the sampler alone at (2048, 2, 512), and at (2048, 2, 256) and (512, 12, 1024): device-event median per batch (a batch is
     the launch and the allocation of its four results), windows/s, GB/s at the 4 x B x leads x L x 4 bytes the call has to move
     (clean and noise rows read, clean and noisy windows written), and the same calls issued back to back.  The kernel's own time
     is what `rocprofv3 --kernel-trace --stats -- python tools/mix_bench.py --models ""` lists for k_mix_batch;
  2. one epoch of U-Net and of RA-LENet training through `train()`, same model, same batch, same number of train and test
     steps, fed by `make_loaders` and fed by the sampler, alternating, `--epochs` times each after one warm-up epoch each: the
     median wall-clock of an epoch (every epoch ends in the `.item()` reads of `train()`, a device synchronise) and windows/s
     over the train AND test windows of the epoch; next to them the model's bare step rate on inputs staged on the device (what
     bench.py reports): a fed epoch can exceed it, since its test batches are forward passes only.

The data are synthetic (ecg_denoise_amd/synth.py; 4096 distinct windows, repeated: the timing does not depend on the samples).
The host loader's arrays hold `--windows` pre-mixed windows, 80 % train / 20 % test as main.py:52-60; the sampler draws from the
same clean windows.

    python tools/mix_bench.py [--windows 40960] [--epochs 5] [--batch 2048]      (writes nothing: one text line per leg, one JSON
                                                                                  line at the end)
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ecg_denoise_amd import NoiseMixSampler, RALENet, UNet, synth  # noqa: E402
from ecg_denoise_amd.data import make_loaders  # noqa: E402
from ecg_denoise_amd.train import train  # noqa: E402

DEV, LEADS, L = "cuda:0", 2, 512
OTHER_SHAPES = ((2048, 2, 256), (512, 12, 1024))      # the sampler alone: a shorter window, and the largest the models use


class HostDataset:
    """`EcgDataset` without the files: .data (noisy) and .ground_data (clean), (N, leads, L) fp32"""

    def __init__(self, noisy, clean):
        self.data, self.ground_data = noisy, clean

    def __len__(self):
        return self.data.shape[0]


def sampler_alone(clean, noises, B, reps, warmup):
    LEADS, L = clean.shape[1:]
    s = NoiseMixSampler(clean, noises, L=L, device=DEV)
    for _ in range(warmup):
        s.batch(B)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        s.batch(B)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    # the same calls back to back: what a training loop that never waits for a batch pays per batch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        s.batch(B)
    torch.cuda.synchronize()
    stream_ms = (time.perf_counter() - t0) / reps * 1e3
    ms = float(np.median(ts))
    nbytes = 4 * B * LEADS * L * 4
    return {"batch": B, "leads": LEADS, "L": L, "event_ms_median": ms, "event_ms_min": float(min(ts)), "event_ms_max": float(max(ts)),
            "windows_per_s": B / ms * 1e3, "GBps_at_4_rows": nbytes / ms / 1e6, "back_to_back_ms": stream_ms,
            "back_to_back_windows_per_s": B / stream_ms * 1e3}


def bare_step(model, B, steps=20, warmup=3):
    g = torch.Generator().manual_seed(2023)
    x, t = torch.randn(B, LEADS, L, generator=g).to(DEV), torch.randn(B, LEADS, L, generator=g).to(DEV)
    model.train()
    for _ in range(warmup):
        model.train_step(x, t, 1e-3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.train_step(x, t, 1e-3)
    torch.cuda.synchronize()
    return B * steps / (time.perf_counter() - t0)


def epoch_seconds(model, B, train_loader, test_loader, out_dir):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train(1, model, B, train_loader, test_loader, model_name="mix_bench", noise_name="mixed", noise_intensity=0, out_dir=out_dir,
          log=lambda *a: None)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=40960)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--models", default="unet,ralenet")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: needs a HIP device")
    B = args.batch
    unique = min(args.windows, 4096)                                   # synthesis is slow on the host: 4096 windows, repeated
    noisy, clean = (np.ascontiguousarray(np.resize(a, (args.windows, LEADS, L)))
                    for a in synth.make_dataset(unique, LEADS, L, "emb", 0.0, 2023))
    noises = {k: synth.make_noise_record(k, LEADS, 650000, seed=4) for k in ("bw", "ma", "em")}
    out = {"tool": "mix_bench", "windows": args.windows, "epochs": args.epochs, "device": torch.cuda.get_device_name(0)}

    out["sampler"] = []
    rng = np.random.default_rng(2023)
    for b, leads, ln in ((B, LEADS, L),) + OTHER_SHAPES:
        bank = clean if (leads, ln) == (LEADS, L) else rng.standard_normal((4096, leads, ln)).astype(np.float32)
        recs = noises if leads == LEADS else rng.standard_normal((3, leads, 650000)).astype(np.float32)
        r = sampler_alone(bank, recs, b, args.reps, 5)
        out["sampler"].append(r)
        print(f"sampler alone ({b}, {leads}, {ln}): {r['event_ms_median']:.4f} ms per batch (min {r['event_ms_min']:.4f}, max "
              f"{r['event_ms_max']:.4f}), {r['windows_per_s']:.3e} windows/s, {r['GBps_at_4_rows']:.0f} GB/s; back to back "
              f"{r['back_to_back_ms']:.4f} ms, {r['back_to_back_windows_per_s']:.3e} windows/s")

    host_train, host_test = make_loaders(HostDataset(noisy, clean), batch_size=B, n_select=args.windows)
    host_train.drop_last = host_test.drop_last = True                  # whole batches on both sides
    n_train, n_test = len(host_train), len(host_test)
    per_epoch = (n_train + n_test) * B
    with tempfile.TemporaryDirectory() as tmp:
        for name in [m for m in args.models.split(",") if m]:         # --models "": the sampler alone (e.g. under a kernel trace)
            make = (lambda: UNet(leads=LEADS, L=L, max_batch=B, device=DEV, seed=2023)) if name == "unet" else \
                   (lambda: RALENet("full", leads=LEADS, L=L, max_batch=B, device=DEV, seed=2023))
            model = make()
            bare = bare_step(model, B)
            s = NoiseMixSampler(clean, noises, L=L, device=DEV)
            dev_test = s.loader(B, n_test, replay=True)
            legs = {"host": lambda: epoch_seconds(model, B, host_train, host_test, tmp),
                    "device": lambda: epoch_seconds(model, B, s.loader(B, n_train), dev_test, tmp)}
            times = {k: [] for k in legs}
            for k in legs:
                legs[k]()                                              # warm-up epoch
            for _ in range(args.epochs):
                for k in legs:                                         # alternating
                    times[k].append(legs[k]())
            row = {"model": name, "batch": B, "train_steps": n_train, "test_steps": n_test, "bare_step_windows_per_s": bare}
            for k, ts in times.items():
                row[k] = {"epoch_s_median": float(np.median(ts)), "epoch_s_min": min(ts), "epoch_s_max": max(ts),
                          "windows_per_s": per_epoch / float(np.median(ts))}
            row["device_over_host"] = row["host"]["epoch_s_median"] / row["device"]["epoch_s_median"]
            out[name] = row
            print(f"{name}: epoch of {n_train} + {n_test} batches of {B}: host loader {row['host']['epoch_s_median'] * 1e3:.1f} ms "
                  f"({row['host']['windows_per_s']:.3e} windows/s), sampler {row['device']['epoch_s_median'] * 1e3:.1f} ms "
                  f"({row['device']['windows_per_s']:.3e} windows/s), x{row['device_over_host']:.2f}; bare train step "
                  f"{bare:.3e} windows/s")
            del model
    print(json.dumps(out))


if __name__ == "__main__":
    main()
