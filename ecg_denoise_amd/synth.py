"""Synthetic 2-lead ECG windows with baseline-wander / muscle / electrode-motion noise.

MIT-BIH / NSTDB are not available offline, so throughput and SNR-improvement runs use this generator:
PQRST beats as sums of Gaussians at 360 Hz, heart rate 50-110 bpm with jitter, one R peak placed inside
the central eighth of the window (so the centred R-wave bias of RA-LENet is meaningful), per-window
z-score (reference `np_norm`, local_utils/local_utils.py:261-266), noise scaled to the target input SNR
with the reference formula scale = sqrt(P_sig / 10^(snr/10) / P_noise) (local_utils/local_utils.py:183-189).
Pure numpy; deterministic for a given seed."""
import numpy as np

FS = 360.0
# (offset from R in s, width in s, amplitude) per lead for P, Q, R, S, T
_WAVES = np.array([
    [(-0.20, 0.025, 0.12), (-0.035, 0.010, -0.10), (0.0, 0.011, 1.00), (0.030, 0.012, -0.22), (0.24, 0.045, 0.28)],
    [(-0.21, 0.028, 0.08), (-0.040, 0.011, -0.05), (0.0, 0.013, 0.65), (0.034, 0.014, -0.35), (0.25, 0.050, 0.18)],
])


def _beats(rng, n, L, leads, truth=None):
    """`truth`: a list that receives, per strip, the R-peak sample indices that fall inside it (no draw depends on it)"""
    t = np.arange(L) / FS
    x = np.zeros((n, leads, L))
    for i in range(n):
        at = []
        rr = 60.0 / rng.uniform(50, 110)
        r0 = (L / 2 + rng.uniform(-L / 16, L / 16)) / FS
        k0 = int(np.floor((0 - r0) / rr)) - 1
        k1 = int(np.ceil((L / FS - r0) / rr)) + 1
        amp = rng.uniform(0.8, 1.2)
        for k in range(k0, k1 + 1):
            rk = r0 + k * rr * (1 + (0 if k == 0 else rng.normal(0, 0.03)))
            at.append(int(np.floor(rk * FS + 0.5)))
            for ld in range(leads):
                for (off, wid, a) in _WAVES[ld % 2]:
                    x[i, ld] += amp * a * np.exp(-0.5 * ((t - rk - off * np.sqrt(rr / 0.8)) / wid) ** 2)
        if truth is not None:
            truth.append(sorted(p for p in at if 0 <= p < L))
    return x


def _band_noise(rng, shape, f_lo, f_hi):
    n = shape[-1]
    spec = np.fft.rfft(rng.standard_normal(shape), axis=-1)
    f = np.fft.rfftfreq(n, 1 / FS)
    spec *= ((f >= f_lo) & (f <= f_hi))
    return np.fft.irfft(spec, n, axis=-1)


def noise(rng, kind, shape):
    """bw: 0.05-0.7 Hz drift; ma: 5-50 Hz bursts; em: steps and spikes; emb: their sum."""
    n, leads, L = shape
    if kind == "bw":
        # drift needs a long support: synthesise 8x the window and cut
        z = _band_noise(rng, (n, leads, 8 * L), 0.05, 0.7)
        return z[..., 3 * L:4 * L]
    if kind == "ma":
        z = _band_noise(rng, shape, 5.0, 50.0)
        env = np.ones(shape)
        for i in range(n):
            c, w = rng.uniform(0, L), rng.uniform(L / 8, L / 2)
            env[i] = 0.3 + np.exp(-0.5 * ((np.arange(L) - c) / w) ** 2)
        return z * env
    if kind == "em":
        z = np.zeros(shape)
        for i in range(n):
            for ld in range(leads):
                for _ in range(rng.integers(1, 4)):
                    p = rng.integers(0, L)
                    z[i, ld, p:] += rng.normal(0, 1.0)
                for _ in range(rng.integers(0, 3)):
                    p = rng.integers(0, L)
                    z[i, ld] += rng.normal(0, 3.0) * np.exp(-0.5 * ((np.arange(L) - p) / 2.0) ** 2)
        return z - z.mean(-1, keepdims=True)
    if kind == "emb":
        out = 0
        for k in ("bw", "ma", "em"):
            z = noise(rng, k, shape)
            out = out + z / np.sqrt((z ** 2).mean((1, 2), keepdims=True) + 1e-12)
        return out
    raise ValueError(kind)


def make_records(R, leads, T, seed=2023, block=4096):
    """-> R synthetic clean records, float32 (R, leads, T), of any length T >= 1 (amplitudes in mV, not z-scored).  A record up
    to `block` samples is one `_beats` strip; a longer one is a sequence of independent strips of `block` samples (each with its
    own heart rate; the rhythm restarts at a strip boundary), so the cost grows with T and not with T^2."""
    rng = np.random.default_rng(seed)
    nb = -(-int(T) // block)
    if nb <= 1:
        x = _beats(rng, R, int(T), leads)
    else:
        x = _beats(rng, R * nb, block, leads).reshape(R, nb, leads, block).transpose(0, 2, 1, 3).reshape(R, leads, nb * block)
    return np.ascontiguousarray(x[..., :T], dtype=np.float32)


def make_records_with_beats(R, leads, T, seed=2023, block=4096):
    """-> (records, beats): `make_records(R, leads, T, seed, block)` bit for bit (the same draws in the same order) and, per
    record, the ascending sample indices of its R peaks (the centre of the R wave's Gaussian, rounded to a sample; the R wave
    peaks there in every lead).  Two properties of the truth list that a scorer must know: beats can fall closer together than a
    detector's refractory period - beat k sits at r0 + k rr (1 + jitter_k) with an independent 3 % jitter of the whole offset
    k rr, so far from the strip's centre two neighbours can nearly coincide (seed 2023 at T = 4096 has a pair 33 samples apart),
    and a beat whose centre lies just outside a strip still leaves part of its waves inside without being listed; and the
    rhythm restarts at every strip boundary (a record longer than `block` is a sequence of independent strips), so the interval
    across a boundary is arbitrary."""
    rng = np.random.default_rng(seed)
    nb = -(-int(T) // block)
    truth = []
    if nb <= 1:
        x = _beats(rng, R, int(T), leads, truth)
        beats = truth
    else:
        x = _beats(rng, R * nb, block, leads, truth).reshape(R, nb, leads, block).transpose(0, 2, 1, 3).reshape(R, leads, nb * block)
        beats = [[b * block + p for b in range(nb) for p in truth[r * nb + b] if b * block + p < T] for r in range(R)]
    return np.ascontiguousarray(x[..., :T], dtype=np.float32), beats


# a ventricular ectopic: no P wave, a wide QRS (Gaussian widths 0.022 - 0.036 s against the normal 0.010 - 0.014 s), the R wave of
# the odd lead upside down, a discordant T (opposite to the R of its lead); same columns as _WAVES.  The deep S keeps enough of
# the complex inside 8 - 24 Hz for `BeatDetector` to find it
_V_WAVES = np.array([
    [(-0.050, 0.022, -0.15), (0.0, 0.022, 1.30), (0.058, 0.026, -0.75), (0.30, 0.060, -0.35)],
    [(-0.050, 0.024, 0.10), (0.0, 0.024, -1.00), (0.062, 0.028, 0.55), (0.30, 0.065, 0.30)],
])


def make_records_with_rhythm(R, leads, T, seed=2023, p_v=0.12, p_s=0.0):
    """-> (records, beats, labels): R synthetic clean records, float32 (R, leads, T), at 360 Hz with ectopic beats, per record
    the ascending sample indices of its R peaks and per beat its label, 0 normal (N), 1 ventricular (V), 2 premature with a
    normal shape (S).  Draws of its own (`make_records` and `make_records_with_beats` keep theirs).  A record is one strip:
    heart rate 50 - 110 bpm, amplitude 0.8 - 1.2 and the waves of `_beats` (`_WAVES`, P and T offsets scaled with the
    square root of the interval), every sinus interval rr (1 + a 3 % jitter).  A beat becomes V with probability `p_v`,
    otherwise S with probability `p_s` - never the first beat of the list and never directly after a V or an S.  Such a beat
    comes early, at 0.55 - 0.75 of the running interval after the beat before it, and is followed by a compensatory pause: the
    sinus beat it pre-empts is dropped and the one after that comes on time.  A V beat has the waves of `_V_WAVES`, an S beat
    the normal ones.  A wave is added within 8 of its widths (beyond them it is below 2e-14 of its height), so the cost grows
    with T."""
    rng = np.random.default_rng(seed)
    T = int(T)
    x = np.zeros((R, leads, T))
    t = np.arange(T) / FS
    beats, labels = [], []
    for i in range(R):
        rr = 60.0 / rng.uniform(50, 110)
        amp = rng.uniform(0.8, 1.2)
        stretch = np.sqrt(rr / 0.8)
        at, lab = [], []
        prev, was_early = -rng.uniform(1.0, 2.0) * rr, True       # (a sinus beat before the record: its T wave may reach in)
        events = [(prev, 0)]
        while prev < T / FS + rr:
            gap = rr * (1 + rng.normal(0, 0.03))
            u, kind = rng.uniform(0.55, 0.75), rng.uniform()
            early = bool(at) and not was_early and kind < p_v + p_s
            if early:
                events.append((prev + u * gap, 1 if kind < p_v else 2))
                gap *= 2                                           # the pre-empted sinus beat is dropped
                if 0 <= int(np.floor(events[-1][0] * FS + 0.5)) < T:
                    at.append(int(np.floor(events[-1][0] * FS + 0.5)))
                    lab.append(events[-1][1])
            prev += gap
            events.append((prev, 0))
            was_early = early
            p = int(np.floor(prev * FS + 0.5))
            if 0 <= p < T:
                at.append(p)
                lab.append(0)
        for rk, kind in events:
            for ld in range(leads):
                for (off, wid, a) in (_V_WAVES if kind == 1 else _WAVES)[ld % 2]:
                    c = rk + off * stretch
                    lo, hi = max(0, int((c - 8 * wid) * FS)), min(T, int((c + 8 * wid) * FS) + 2)
                    if lo < hi:
                        x[i, ld, lo:hi] += amp * a * np.exp(-0.5 * ((t[lo:hi] - c) / wid) ** 2)
        beats.append(at)
        labels.append(lab)
    return x.astype(np.float32), beats, labels


def make_beats_with_hrv(R, T, fs=360, seed=2023, lf=0.04, hf=0.02, p_v=0.0, p_s=0.0, bpm=(55.0, 95.0)):
    """-> (beats, labels): per record the strictly ascending sample indices in [0, T) of the beats of a rhythm with a known
    variability, at rate `fs`, and per beat its label, 0 normal (N), 1 ventricular (V), 2 premature with a normal shape (S).  No
    signal is generated.  Draws of its own (the other generators keep theirs).  Per record a mean heart rate from `bpm` (beats
    per minute, uniform) gives rr0, and a sinus beat at time t is followed by the next after
    rr0 + lf sin(2 pi 0.1 t + a) + hf sin(2 pi 0.25 t + b) seconds (a, b uniform phases): `lf` and `hf` are the amplitudes, in
    seconds, of the modulation at 0.1 Hz (the LF band) and at 0.25 Hz (the HF band), so the NN series carries about lf^2 / 2 and
    hf^2 / 2 of power there.  A beat becomes V with probability `p_v`, otherwise S with probability `p_s` - never the first beat
    and never directly after a V or an S; it comes at 0.55 - 0.75 of the interval and the sinus beat it pre-empts is dropped (a
    compensatory pause), as in `make_records_with_rhythm`."""
    rng = np.random.default_rng(seed)
    T, fs = int(T), float(fs)
    beats, labels = [], []
    for _ in range(R):
        rr0 = 60.0 / rng.uniform(*bpm)
        a, b = rng.uniform(0, 2 * np.pi, 2)
        t, at, lab, was_early = rng.uniform(0, rr0), [], [], True
        while t * fs < T:
            p = int(np.floor(t * fs + 0.5))
            if p < T and (not at or p > at[-1]):
                at.append(p)
                lab.append(0)
            gap = rr0 + lf * np.sin(2 * np.pi * 0.1 * t + a) + hf * np.sin(2 * np.pi * 0.25 * t + b)
            u, kind = rng.uniform(0.55, 0.75), rng.uniform()
            early = len(at) > 0 and not was_early and kind < p_v + p_s
            if early:
                pe = int(np.floor((t + u * gap) * fs + 0.5))
                if at[-1] < pe < T:
                    at.append(pe)
                    lab.append(1 if kind < p_v else 2)
                gap *= 2
            was_early = early
            t += gap
        beats.append(at)
        labels.append(lab)
    return beats, labels


def make_records_with_af(R, leads, T, seed=2023, cv=(0.15, 0.25), f_amp=(0.03, 0.06), f_hz=(4.0, 9.0), share=(0.3, 0.6)):
    """-> (records, beats, labels, episodes): R synthetic clean records, float32 (R, leads, T), at 360 Hz, each sinus rhythm, then
    one episode of atrial fibrillation (AF), then sinus rhythm again; per record the ascending sample indices of its R peaks, per
    beat its label (all 0: AF beats have the normal QRS) and `episodes`, per record the list [(position of the first AF beat,
    position of the first sinus beat after it, or T if that one lies beyond the record)].  Draws of its own (the other generators
    keep theirs).  A record is one strip: heart rate 50 - 110 bpm, amplitude 0.8 - 1.2 and the waves of `_beats` (`_WAVES`, P and
    T offsets scaled with the square root of the sinus interval), every sinus interval rr (1 + a 3 % jitter).  The episode takes
    `share` (uniform) of the record and starts at 0.1 .. 0.9 - share of it.  Inside it the intervals are
    max(0.3 s, rr_af (1 + cv N(0, 1))) with rr_af drawn from 70 - 140 bpm and `cv` uniform; the beats have no P wave; and each
    lead carries a fibrillatory wave a sin(2 pi f t + phi + 0.8 sin(2 pi 0.23 t + psi)) - amplitude `f_amp` in mV, frequency
    `f_hz`, a slow phase wobble - from half an interval behind the last sinus beat to half an interval in front of the next,
    faded in and out over 0.1 s.  A wave is added within 8 of its widths, as in `make_records_with_rhythm`."""
    rng = np.random.default_rng(seed)
    T = int(T)
    x = np.zeros((R, leads, T))
    t = np.arange(T) / FS
    dur = T / FS
    beats, labels, episodes = [], [], []
    for i in range(R):
        rr = 60.0 / rng.uniform(50, 110)
        amp = rng.uniform(0.8, 1.2)
        stretch = np.sqrt(rr / 0.8)
        sh = rng.uniform(*share)
        ta = rng.uniform(0.1, max(0.1, 0.9 - sh)) * dur
        tb = min(ta + sh * dur, dur)
        rr_af, c = 60.0 / rng.uniform(70, 140), rng.uniform(*cv)
        prev = -rng.uniform(1.0, 2.0) * rr                       # (a sinus beat before the record: its T wave may reach in)
        events = [(prev, 0)]
        while True:                                              # sinus rhythm up to the episode
            gap = rr * (1 + rng.normal(0, 0.03))
            if prev + gap > ta:
                break
            prev += gap
            events.append((prev, 0))
        f_on = prev
        first = None
        while first is None or prev < tb:                        # the episode: at least one beat
            prev += max(0.3, rr_af * (1 + c * rng.normal(0, 1)))
            events.append((prev, 3))
            if first is None:
                first, f_on = prev, 0.5 * (f_on + prev)
        last = prev
        prev += rr * (1 + rng.normal(0, 0.03))
        back, f_off = prev, 0.5 * (last + prev)
        events.append((prev, 0))
        while prev < dur + rr:
            prev += rr * (1 + rng.normal(0, 0.03))
            events.append((prev, 0))
        for rk, kind in events:
            for ld in range(leads):
                for (off, wid, a) in _WAVES[ld % 2][1 if kind == 3 else 0:]:
                    cen = rk + off * stretch
                    lo, hi = max(0, int((cen - 8 * wid) * FS)), min(T, int((cen + 8 * wid) * FS) + 2)
                    if lo < hi:
                        x[i, ld, lo:hi] += amp * a * np.exp(-0.5 * ((t[lo:hi] - cen) / wid) ** 2)
        lo, hi = max(0, int(f_on * FS)), min(T, int(f_off * FS) + 1)
        for ld in range(leads):
            a, f = rng.uniform(*f_amp), rng.uniform(*f_hz)
            phi, psi = rng.uniform(0, 2 * np.pi, 2)
            if lo < hi:
                ts = t[lo:hi]
                fade = np.clip(np.minimum(ts - f_on, f_off - ts) / 0.1, 0.0, 1.0)
                x[i, ld, lo:hi] += a * fade * np.sin(2 * np.pi * f * ts + phi + 0.8 * np.sin(2 * np.pi * 0.23 * ts + psi))
        at = [int(np.floor(rk * FS + 0.5)) for rk, _ in events]
        beats.append([p for p in at if 0 <= p < T])
        labels.append([0] * len(beats[-1]))
        episodes.append([(min(max(int(np.floor(first * FS + 0.5)), 0), T), min(int(np.floor(back * FS + 0.5)), T))])
    return x.astype(np.float32), beats, labels, episodes


def make_noise_record(kind, leads, Tn, seed=2023):
    """-> one synthetic noise record, float32 (leads, Tn), of kind bw / ma / em / emb (`noise`): the stand-in for an NSTDB
    record that `mix_records` cuts its segments from."""
    return np.ascontiguousarray(noise(np.random.default_rng(seed), kind, (1, leads, int(Tn)))[0], dtype=np.float32)


def make_dataset(n=10000, leads=2, L=256, noise_name="emb", snr_db=0.0, seed=2023):
    """-> (noisy, clean) float32 arrays of shape (n, leads, L); the on-disk counterpart is
    data/dict_data/{m4,m2,0,p2,p4}/{bw,ma,em,emb}.npy + data/dict_data/ecg.npy (data_utils.py:92-117)."""
    rng = np.random.default_rng(seed)
    clean = _beats(rng, n, L, leads)
    clean = clean - clean.mean(-1, keepdims=True)
    clean = clean / clean.std(-1, keepdims=True)                      # np_norm over the window
    z = noise(rng, noise_name, (n, leads, L))
    p_sig = (clean ** 2).mean((1, 2), keepdims=True)
    p_noise = (z ** 2).mean((1, 2), keepdims=True)
    scale = np.sqrt(p_sig / (10 ** (snr_db / 10)) / p_noise)           # single_snr_noise_add
    return (clean + scale * z).astype(np.float32), clean.astype(np.float32)


def split_8000_2000(noisy, clean, seed=2023):
    """main.py:52-58 protocol: 80/20 split of the selected windows (own RNG, documented deviation)."""
    idx = np.random.default_rng(seed).permutation(len(noisy))
    k = int(0.8 * len(idx))
    return (noisy[idx[:k]], clean[idx[:k]]), (noisy[idx[k:]], clean[idx[k:]])
