"""Frozen-BatchNorm step against the batch-statistics step (model.freeze_bn) on one MI355X: the same model, the same
inputs, one `train_step` of each mode timed in alternating rounds, so that whatever else the host does touches both alike.
Configurations: RA-LENet "full" 2 x 512 and U-Net 2 x 512, each at batch 4 (fine-tuning on a few windows) and 2048
(the training batch).  One JSON line per configuration: median and spread (min .. max) over the rounds, in ms per step.

    python tools/finetune_bench.py [--rounds 7] [--steps 30] [--warmup 5] [--only ralenet|unet] [--batch 4 2048]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ecg_denoise_amd import RALENet, UNet  # noqa: E402

LEADS, L = 2, 512


def make(net, B):
    if net == "ralenet":
        return RALENet("full", leads=LEADS, L=L, max_batch=B, device="cuda:0", seed=1)
    return UNet(leads=LEADS, L=L, max_batch=B, device="cuda:0", seed=1)


def timed(model, x, t, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model.train_step(x, t, 1e-5)       # (a small rate: 2 x rounds x steps updates leave the model where it started)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def run(net, B, rounds, steps, warmup):
    model = make(net, B).train()
    g = torch.Generator().manual_seed(2023)
    x = torch.randn(B, LEADS, L, generator=g).cuda()
    t = torch.randn(B, LEADS, L, generator=g).cuda()
    ms = {False: [], True: []}
    for frozen in (False, True):           # every kernel of both modes is loaded before the first timed round
        model.freeze_bn(frozen)
        timed(model, x, t, warmup)
    for _ in range(rounds):
        for frozen in (False, True):
            model.freeze_bn(frozen)
            ms[frozen].append(timed(model, x, t, steps))
    model.freeze_bn(False)
    out = {"model": net, "leads": LEADS, "L": L, "batch": B, "rounds": rounds, "steps_per_round": steps}
    for frozen, key in ((False, "batch_stats"), (True, "frozen")):
        v = ms[frozen]
        out[key + "_ms"] = round(statistics.median(v), 4)
        out[key + "_min_ms"], out[key + "_max_ms"] = round(min(v), 4), round(max(v), 4)
    out["frozen_over_batch_stats"] = round(out["frozen_ms"] / out["batch_stats_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("ralenet", "unet"), default=None)
    ap.add_argument("--batch", type=int, nargs="+", default=[4, 2048])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("finetune_bench: no HIP device (a step time is measured on the GPU or not at all)")
    for net in ("ralenet", "unet"):
        if a.only in (None, net):
            for B in a.batch:
                print(json.dumps(run(net, B, a.rounds, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
