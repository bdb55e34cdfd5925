"""Noise-stress evaluation of streamed denoising on synthetic records: the reference's experiment grid (run.sh: models x
{bw, ma, em, emb} x {-4, -2, 0, 2, 4 dB}, one `snr:..., rmse:...` line each) on long records through `StreamingDenoiser`.

For every noise kind ONE `StreamingDenoiser.evaluate` call covers the whole intensity sweep: the records of the group are split
over the five intensities through per-record SNRs (`--records` per intensity, so 5 x `--records` records of `--T` samples per
call).  Per (kind, intensity) the tool prints the reference-format line (`RecordScores.output_line`) of the model and of the
classical baseline - `wavelet_denoise` on the same noisy records, cut into rows of `--wavelet-L` samples, scored through
`score_records` with the same tile length - and at the end one JSON object: per cell SNR in / out / improvement and RMSE (mean
over the tiles of L samples, the reference's protocol, and over whole records), for both.

The JSON also carries device-event timings (`--time-shapes`, default "64x2x650000,16x12x650000": records x leads x samples; 2 leads
run `--model`, 12 leads a NewRALE around RALENet("full", L = 256)): after a warm-up call of the same shape, `mix`, `denoise` and
`score` on their own, and `evaluate` against `denoise` alone on the same noisy records, the two alternating in one process
(`--reps` pairs, medians).  `overhead_share` = (evaluate - denoise) / evaluate; GB/s are algorithmic (bytes from the shapes: mix
24 B, score 12 B per sample and lead).  Without `--ckpt` the model has its seeded initial weights: the timings and the plumbing
are meaningful, the dB are not those of a trained model.  Needs a HIP device: there is no fallback.

`--beats` adds what the protocol was built to ask - does denoising give back the beats the noise destroyed: per cell one more
line and a "beats" entry in the JSON with sensitivity (Se), positive predictivity (+P) and F1 of `BeatDetector` on the noisy and
on the denoised records against its detections on the clean ones (`evaluate_beats`, 150 ms).  Without the flag the output is
what it was.

`--classes` asks the reference's own downstream question (test_cls.py) of the deterministic beat classifier: per cell one more
line and a "classes" entry in the JSON with the N / V / S / unclassified counts of `BeatClassifier` on the clean, the noisy and
the denoised records at the clean records' detections, and accuracy, precision and F1 of the noisy and of the denoised V
decisions against the clean ones (`evaluate_rhythm`; NaN where a ratio has no denominator).  Without the flag the output is
what it was.

`--fft` adds the reference's other classical baseline, the model "fft" of test_cls.py: `fft_denoise` on the same noisy records
through `ClassicalDenoiser("fft", --fft-L)` (windows of `--fft-L` samples, default 1000 as in test_cls.py:246; the leads of a
window share one cutoff), scored like the wavelet row: per cell one more reference-format line and an "fft" entry in the JSON.
Without the flag the output is what it was.

`--hrv` asks the third question, are the rhythm statistics back: per cell one more line and an "hrv" entry in the JSON with the
mean absolute error of heart rate, SDNN, RMSSD and log(LF/HF) of the noisy and of the denoised records against the clean ones,
each record detected, classified and analysed on its own (`evaluate_hrv`; windows of `--hrv-win` seconds every `--hrv-hop`
seconds; NaN where no window has all three values).  Without the flag the output is what it was.

`--intervals` asks the fourth question, are the intervals back: per cell one more line and an "intervals" entry in the JSON
with, for the noisy and for the denoised records, the share of the beats whose QRS duration (and whose QT) can be measured in the
clean record and can be measured here too, and the mean absolute error of QRS duration and of QT in ms over the beats measurable
in both - `BeatDelineator` at the clean records' detections (`evaluate_intervals`; NaN where there is no such beat).  Without
the flag the output is what it was.

`--templates` asks the fifth question, is the shape of the beat back: per cell one more line and a "templates" entry in the JSON
with, for the noisy and for the denoised records, the RMSE of the median beat of every `--template-win` seconds against the clean
records' median beat at the same beats and classes, pooled over the windows with at least three used beats, and the pooled
shares and errors of QRS duration and QT measured on the median beats (`evaluate_templates`; NaN where there is no such
window).  Without the flag the output is what it was.

`--pst` asks the sixth question, are the P wave and the ST level back: per cell one more line and a "pst" entry in the JSON
with, for the noisy and for the denoised records, the share of the clean records' P waves that are still found, the mean absolute
error of the PR interval in ms over the beats that have a P wave in both, and that of the ST level per lead over the beats that
have one in both - `PStMeasurer` on `BeatDelineator` at the clean records' detections (`evaluate_pst`; NaN where there is no such
beat; the ST error is in the unit of the mixed records, which `mix_records` z-scores).  Without the flag the output is what it was.

`--af` asks the seventh question, is the rhythm diagnosis back: a pass of its own over records with one episode of atrial
fibrillation each (`synth.make_records_with_af`, the same count, length, noise, SNRs and offsets as the grid's), every condition
detected, classified, delineated, measured and analysed on its own (`evaluate_af` against the generator's episodes; windows of
`--af-win` seconds every `--af-hop` seconds).  Per cell one more line and an "af" entry in the JSON with tp, fp, fn, tn,
sensitivity and specificity of the AF bit per window for the clean, the noisy and the denoised records (NaN where a ratio has
no denominator).  The analysis' defaults were chosen on synthetic data only.  Without the flag the output is what it was.

    python tools/stress_eval.py [--model full|nra|mlp|unet|acdae|danet|newrale] [--ckpt state_dict.pth] [--L 512]
                                [--records 4] [--T 65000] [--overlap 0] [--batch 4096] [--time-shapes ...] [--reps 5] [--beats]
                                [--classes] [--fft] [--fft-L 1000] [--hrv] [--hrv-win 60] [--hrv-hop 30] [--intervals]
                                [--templates] [--template-win 10] [--pst] [--af] [--af-win 30] [--af-hop 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ecg_denoise_amd import (ACDAE, ClassicalDenoiser, DANet, NewRALE, RALENet, UNet, af_scores, evaluate_af,  # noqa: E402
                             evaluate_beats, evaluate_hrv, evaluate_intervals, evaluate_pst, evaluate_rhythm, evaluate_templates,
                             interval_scores, mix_records, pst_scores, score_records, synth, wavelet_denoise)
from ecg_denoise_amd.data import NOISE_TYPES, TRUE_NOISE  # noqa: E402
from ecg_denoise_amd.infer import StreamingDenoiser  # noqa: E402

DEV = "cuda:0"


def make_model(name, L, batch, ckpt=None):
    kw = dict(L=L, max_batch=batch, train=False, device=DEV)
    if name in ("full", "nra", "mlp"):
        m = RALENet(name, leads=2, seed=777, **kw)
    elif name == "unet":
        m = UNet(leads=2, seed=777, **kw)
    elif name == "acdae":
        m = ACDAE(seed=777, **kw)
    elif name == "danet":
        m = DANet(seed=777, **kw)
    elif name == "newrale":
        m = NewRALE(RALENet("full", leads=2, seed=777, **kw), seed=778)
    else:
        raise SystemExit(f"stress_eval: unknown model {name}")
    if ckpt:
        m.load_state_dict(torch.load(ckpt, map_location="cpu"))
    return m.eval()


def _records(R, leads, T, seed, distinct=4):
    """R records on the device; at most `distinct` different ones are synthesised, the others repeat them (the timing legs
    need the shape, not the variety)"""
    base = torch.tensor(synth.make_records(min(R, distinct), leads, T, seed=seed), device=DEV)
    return base.repeat(-(-R // base.shape[0]), 1, 1)[:R].contiguous()


def _row(sc):
    """all-tiles means (reference protocol) and the mean of the per-record values, as plain floats"""
    s = sc.summary()
    rec = sc.per_record.mean(0).tolist()
    s.update(record_snr_in_db=rec[0], record_snr_out_db=rec[1], record_rmse_out=rec[3])
    return s


def _subset(sc, idx, window):
    """the scores of the records idx of a group as a RecordScores of their own (the all-tiles row formed again)"""
    from ecg_denoise_amd.evaluate import RecordScores
    pw = sc.per_window[idx]
    wm = torch.cat([sc.window_mean[idx], pw.reshape(-1, 4).mean(0, keepdim=True)])
    return RecordScores(sc.per_lead[idx], sc.per_record[idx], pw, wm, window)


def _classes_cell(ev, idx):
    """the records idx of an `evaluate_rhythm` result -> counts per class and the three scores, noisy and denoised"""
    from ecg_denoise_amd.rhythm import _score
    rows = torch.zeros(ev.mask.shape[0], dtype=torch.bool, device=ev.mask.device)
    rows[idx] = True
    mask = ev.mask & rows[:, None]
    truth = (ev.clean.label[mask] == 1).long()
    out = {k: dict(zip(("N", "V", "S", "unclassified"), c.counts()[idx].sum(0).tolist()))
           for k, c in (("clean", ev.clean), ("noisy", ev.noisy), ("denoised", ev.denoised))}
    out["scored_beats"] = int(mask.sum())
    out["noisy"].update(_score(ev.noisy.logits(mask)[0], truth))
    out["denoised"].update(_score(ev.denoised.logits(mask)[0], truth))
    return out


def _hrv_cell(ev, idx):
    """the records idx of an `evaluate_hrv` result -> per metric the windows compared and the two mean absolute errors"""
    from ecg_denoise_amd.hrv import METRICS, _metric
    rows = torch.from_numpy(np.isin(ev.clean.index[:, 0], idx.cpu().numpy())).to(ev.clean.stats.device)
    out = {"windows": {}, "noisy": {}, "denoised": {}}
    for m in METRICS:
        c, a, b = (_metric(h, m) for h in (ev.clean, ev.noisy, ev.denoised))
        ok = rows & torch.isfinite(c) & torch.isfinite(a) & torch.isfinite(b)
        out["windows"][m] = int(ok.sum())
        for key, v in (("noisy", a), ("denoised", b)):
            out[key][m] = float((v[ok] - c[ok]).abs().mean()) if out["windows"][m] else float("nan")
    return out


def _intervals_cell(ev, idx):
    """the records idx of an `evaluate_intervals` result -> the pooled shares and errors, noisy and denoised"""
    return {key: interval_scores(ev.clean, f, rows=idx)[2] for key, f in (("noisy", ev.noisy), ("denoised", ev.denoised))}


def _pst_cell(ev, idx):
    """the records idx of an `evaluate_pst` result -> the pooled share and errors, noisy and denoised"""
    return {key: pst_scores(ev.clean, p, rows=idx)[2] for key, p in (("noisy", ev.noisy), ("denoised", ev.denoised))}


def _af_cell(ev, idx):
    """the records idx of an `evaluate_af` result -> per condition the AF bit's tp, fp, fn, tn, sensitivity and specificity"""
    rows = np.isin(ev.clean.index[:, 0], idx.cpu().numpy())
    return {key: af_scores(r.af.cpu().numpy(), ev.positive, ev.scored & rows)
            for key, r in (("clean", ev.clean), ("noisy", ev.noisy), ("denoised", ev.denoised))}


def _templates_cell(ev, idx):
    """the records idx of an `evaluate_templates` result -> per condition the pooled RMSE against the clean median beats, how
    many windows it is taken over, and the pooled interval shares and errors"""
    nw = ev.clean.used.shape[1]
    rows = (idx[:, None] * nw + torch.arange(nw, device=idx.device)).reshape(-1)
    out = {}
    for key in ("noisy", "denoised"):
        r = ev.rmse[key][idx]
        ok = torch.isfinite(r)
        out[key] = dict(interval_scores(ev.fiducials["clean"], ev.fiducials[key], rows=rows)[2], windows=int(ok.sum()),
                        rmse=float(torch.sqrt((r[ok] ** 2).mean())) if bool(ok.any()) else float("nan"))
    return out


def grid(args, model, name):
    sd = StreamingDenoiser(model, batch=args.batch, overlap=args.overlap, use_graph=True)
    leads, n_int = sd.leads, len(TRUE_NOISE)
    R = args.records * n_int
    rec = _records(R, leads, args.T, seed=2023, distinct=R)
    snrs = [float(TRUE_NOISE[r // args.records]) for r in range(R)]
    Lw = args.wavelet_L
    cells, lines = [], []
    import random
    for kind in NOISE_TYPES:
        noise = torch.tensor(synth.make_noise_record(kind, leads, args.T + 4096, seed=7), device=DEV)
        rng = random.Random(2023)
        offsets = [rng.randint(0, 4096 - 1) for _ in range(R)]
        sc = sd.evaluate(rec, noise, snrs, offsets=offsets)
        noisy, clean = mix_records(rec, noise, snrs, offsets=offsets)
        nrow = args.T // Lw * Lw                      # the baseline takes rows of an even length <= 8192
        wav = wavelet_denoise(noisy[..., :nrow].reshape(R, leads, nrow // Lw, Lw).reshape(-1, Lw)).reshape(R, leads, nrow)
        sw = score_records(clean[..., :nrow].contiguous(), wav, noisy[..., :nrow].contiguous(), window=sd.L)
        sf = score_records(clean, ClassicalDenoiser("fft", args.fft_L, device=DEV).denoise(noisy), noisy, window=sd.L) if args.fft else None
        ev = evaluate_beats(sd, rec, noise, snrs, offsets=offsets) if args.beats else None
        evc = evaluate_rhythm(sd, rec, noise, snrs, offsets=offsets) if args.classes else None
        evh = None
        if args.hrv:
            from ecg_denoise_amd import HrvAnalyzer
            evh = evaluate_hrv(sd, rec, noise, snrs, offsets=offsets,
                               analyzer=HrvAnalyzer(win_s=args.hrv_win, hop_s=args.hrv_hop, device=DEV))
        evi = evaluate_intervals(sd, rec, noise, snrs, offsets=offsets) if args.intervals else None
        evt = None
        if args.templates:
            from ecg_denoise_amd import MedianBeat
            evt = evaluate_templates(sd, rec, noise, snrs, offsets=offsets,
                                     averager=MedianBeat(win_s=args.template_win, hop_s=args.template_win, device=DEV))
        evp = evaluate_pst(sd, rec, noise, snrs, offsets=offsets) if args.pst else None
        eva = None
        if args.af:
            from ecg_denoise_amd import ArrhythmiaAnalyzer
            xa, _, _, episodes = synth.make_records_with_af(R, leads, args.T, seed=2023)
            eva = evaluate_af(sd, torch.tensor(xa, device=DEV), noise, snrs, truth=episodes, offsets=offsets,
                              analyzer=ArrhythmiaAnalyzer(win_s=args.af_win, hop_s=args.af_hop, device=DEV))
        for i, snr in enumerate(TRUE_NOISE):
            idx = torch.arange(i * args.records, (i + 1) * args.records, device=DEV)
            a, b = _subset(sc, idx, sd.L), _subset(sw, idx, sd.L)
            lines.append(a.output_line(name, 0, kind, snr))
            lines.append(b.output_line("wavelet", 0, kind, snr))
            cells.append({"noise": kind, "intensity": snr, "model": _row(a), "wavelet": _row(b)})
            if sf is not None:
                f = _subset(sf, idx, sd.L)
                lines.append(f.output_line("fft", 0, kind, snr))
                cells[-1]["fft"] = _row(f)
            if ev is not None:
                bn, bd = (type(v)(v.counts[idx], v.tol).pooled for v in (ev.noisy, ev.denoised))
                cells[-1]["beats"] = {"noisy": bn, "denoised": bd}
                col = lambda d: f"Se {d['sensitivity']:.4f} +P {d['ppv']:.4f} F1 {d['f1']:.4f} (tp {d['tp']} fp {d['fp']} fn {d['fn']})"
                lines.append(f"{name}_0_{kind}_intensity{snr}:beats: noisy {col(bn)}, denoised {col(bd)}\n")
            if evc is not None:
                cc = _classes_cell(evc, idx)
                cells[-1]["classes"] = cc
                col = lambda d: (f"acc {d['acc']:.4f} precision {d['precision']:.4f} F1 {d['f1']:.4f} "
                                 f"(N {d['N']} V {d['V']} S {d['S']} unclassified {d['unclassified']})")
                lines.append(f"{name}_0_{kind}_intensity{snr}:classes: clean V {cc['clean']['V']} of {cc['scored_beats']} scored, "
                             f"noisy {col(cc['noisy'])}, denoised {col(cc['denoised'])}\n")
            if evh is not None:
                hc = _hrv_cell(evh, idx)
                cells[-1]["hrv"] = hc
                col = lambda d: (f"hr {d['hr']:.3f} bpm sdnn {1e3 * d['sdnn']:.2f} ms rmssd {1e3 * d['rmssd']:.2f} ms "
                                 f"log(lf/hf) {d['log_lf_hf']:.3f}")
                lines.append(f"{name}_0_{kind}_intensity{snr}:hrv: mean absolute error over {hc['windows']['hr']} windows, "
                             f"noisy {col(hc['noisy'])}, denoised {col(hc['denoised'])}\n")
            if evi is not None:
                ic = _intervals_cell(evi, idx)
                cells[-1]["intervals"] = ic
                col = lambda d: (f"qrs {d['qrs_share']:.4f} of the clean beats, error {d['qrs_mae_ms']:.2f} ms over {d['qrs_beats']}; "
                                 f"qt {d['qt_share']:.4f}, error {d['qt_mae_ms']:.2f} ms over {d['qt_beats']}")
                lines.append(f"{name}_0_{kind}_intensity{snr}:intervals: noisy {col(ic['noisy'])}, denoised {col(ic['denoised'])}\n")
            if evt is not None:
                tc = _templates_cell(evt, idx)
                cells[-1]["templates"] = tc
                col = lambda d: (f"rmse {d['rmse']:.4f} over {d['windows']} median beats; qrs {d['qrs_share']:.4f} of the clean ones, "
                                 f"error {d['qrs_mae_ms']:.2f} ms; qt {d['qt_share']:.4f}, error {d['qt_mae_ms']:.2f} ms")
                lines.append(f"{name}_0_{kind}_intensity{snr}:templates: noisy {col(tc['noisy'])}, denoised {col(tc['denoised'])}\n")
            if evp is not None:
                pc = _pst_cell(evp, idx)
                cells[-1]["pst"] = pc
                col = lambda d: (f"p {d['p_share']:.4f} of the clean P waves, pr error {d['pr_mae_ms']:.2f} ms over {d['p_beats']}; "
                                 f"st error {' '.join(f'{v:.4f}' for v in d['st_mae'])} over {d['st_beats']}")
                lines.append(f"{name}_0_{kind}_intensity{snr}:pst: noisy {col(pc['noisy'])}, denoised {col(pc['denoised'])}\n")
            if eva is not None:
                ac = _af_cell(eva, idx)
                cells[-1]["af"] = ac
                col = lambda d: (f"Se {d['sensitivity']:.4f} Sp {d['specificity']:.4f} "
                                 f"(tp {d['tp']} fp {d['fp']} fn {d['fn']} tn {d['tn']})")
                lines.append(f"{name}_0_{kind}_intensity{snr}:af: clean {col(ac['clean'])}, noisy {col(ac['noisy'])}, "
                             f"denoised {col(ac['denoised'])}\n")
    return cells, lines


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts


def timing(args, R, leads, T, model, name):
    sd = StreamingDenoiser(model, batch=args.batch, overlap=args.overlap, use_graph=True)
    rec = _records(R, leads, T, seed=5, distinct=1 if leads > 2 else 4)
    noise = torch.tensor(synth.make_noise_record("ma", leads, T + 4096, seed=9), device=DEV)
    snrs = [float(TRUE_NOISE[r % len(TRUE_NOISE)]) for r in range(R)]
    offsets = [(r * 997) % 4096 for r in range(R)]
    noisy, clean = mix_records(rec, noise, snrs, offsets=offsets)
    out = sd.denoise(noisy)                                   # warm-up: plan + graph of this shape
    score_records(clean, out, noisy, window=sd.L)
    sd.evaluate(rec, noise, snrs, offsets=offsets)
    torch.cuda.synchronize()
    leg = {"model": name, "records": R, "leads": leads, "T": T, "L": sd.L, "overlap": args.overlap,
           "windows": R * sd.windows_per_record(T)}
    leg["mix_ms"], _ = _median_ms(lambda: mix_records(rec, noise, snrs, offsets=offsets), args.reps)
    leg["score_ms"], _ = _median_ms(lambda: score_records(clean, out, noisy, window=sd.L), args.reps)
    ev, dn = [], []
    for _ in range(args.reps):                                # alternating, one process
        dn.append(_median_ms(lambda: sd.denoise(noisy, copy=False), 1)[0])
        ev.append(_median_ms(lambda: sd.evaluate(rec, noise, snrs, offsets=offsets), 1)[0])
    leg["denoise_ms"], leg["evaluate_ms"] = float(np.median(dn)), float(np.median(ev))
    leg["denoise_ms_all"], leg["evaluate_ms_all"] = dn, ev
    leg["overhead_share"] = (leg["evaluate_ms"] - leg["denoise_ms"]) / leg["evaluate_ms"]
    elems = R * leads * T
    leg["mix_GBps"] = 24 * elems / leg["mix_ms"] / 1e6        # rec + noise read twice, noisy + clean written
    leg["score_GBps"] = 12 * elems / leg["score_ms"] / 1e6    # clean, out, noisy read once
    leg["us_per_window"] = {k: 1e3 * leg[k + "_ms"] / leg["windows"] for k in ("mix", "score", "denoise", "evaluate")}
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="full")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--records", type=int, default=4, help="records per intensity in the grid")
    ap.add_argument("--T", type=int, default=65000)
    ap.add_argument("--overlap", type=int, default=0)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--wavelet-L", type=int, default=1024)
    ap.add_argument("--time-shapes", default="64x2x650000,16x12x650000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--beats", action="store_true", help="add Se / +P / F1 of beat detection, noisy and denoised")
    ap.add_argument("--classes", action="store_true", help="add beat classes (N / V / S) and acc / precision / F1, noisy and denoised")
    ap.add_argument("--fft", action="store_true", help="add the FFT-threshold baseline (the model 'fft') beside the wavelet one")
    ap.add_argument("--fft-L", type=int, default=1000)
    ap.add_argument("--hrv", action="store_true", help="add the errors of heart rate, SDNN, RMSSD and log(LF/HF), noisy and denoised")
    ap.add_argument("--intervals", action="store_true", help="add the shares and errors of QRS duration and QT, noisy and denoised")
    ap.add_argument("--templates", action="store_true", help="add the RMSE and the intervals of the median beats, noisy and denoised")
    ap.add_argument("--template-win", type=int, default=10)
    ap.add_argument("--pst", action="store_true", help="add the share of P waves and the errors of PR and of the ST level, noisy and denoised")
    ap.add_argument("--af", action="store_true", help="add sensitivity and specificity of the AF flag per window on records with AF episodes")
    ap.add_argument("--af-win", type=int, default=30)
    ap.add_argument("--af-hop", type=int, default=10)
    ap.add_argument("--hrv-win", type=int, default=60)
    ap.add_argument("--hrv-hop", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stress_eval: needs a HIP device")
    res = {"tool": "stress_eval", "model": args.model, "ckpt": args.ckpt, "trained": bool(args.ckpt), "L": args.L,
           "records_per_intensity": args.records, "T": args.T, "overlap": args.overlap, "grid": [], "timing": []}
    model = make_model(args.model, args.L, args.batch, args.ckpt)
    res["grid"], lines = grid(args, model, args.model)
    sys.stdout.write("".join(lines))
    for shape in [s for s in args.time_shapes.split(",") if s]:
        R, leads, T = (int(v) for v in shape.split("x"))
        own = StreamingDenoiser(model).leads == leads
        m = model if own else make_model("newrale" if leads == 12 else "full", 256 if leads == 12 else args.L, args.batch)
        res["timing"].append(timing(args, R, leads, T, m, args.model if own else ("newrale" if leads == 12 else "full")))
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
