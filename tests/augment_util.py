"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of ral_mix_batch (include/ralenet.h): the Philox4x32-10 draw in exact integer
arithmetic and the z-score + SNR mix in float64, rounded once to fp32.  Written from the header's text, not from the kernel."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (Python ints) -> 4 words"""
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def draw_ref(seed, first, B, N, Lsrc, L, Tn, cum, snr_lo, snr_hi):
    """-> draws (B, 4) int64 (row, start, kind, offset) and snr_db (B,) float64 of ordinals first .. first + B - 1 (mod 2^64)"""
    key = (seed & MASK, (seed >> 32) & MASK)
    K = len(cum)
    draws = np.empty((B, 4), dtype=np.int64)
    snr = np.empty(B, dtype=np.float64)
    for i in range(B):
        g = (first + i) & (2 ** 64 - 1)
        a = philox4x32_10((g & MASK, g >> 32, 0, 0), key)
        bq = philox4x32_10((g & MASK, g >> 32, 1, 0), key)
        kind = next((k for k in range(K - 1) if a[2] < cum[k]), K - 1)
        draws[i] = ((a[0] * N) >> 32, (a[1] * (Lsrc - L + 1)) >> 32, kind, (bq[0] * (Tn - L + 1)) >> 32)
        snr[i] = np.float64(snr_lo) + (np.float64(snr_hi) - np.float64(snr_lo)) * (np.float64(a[3]) * 2.0 ** -32)
    return draws, snr


def mix_ref(bank, noise, draws, snr_db, L):
    """bank (N, leads, Lsrc), noise (K, leads, Tn) fp32 arrays; draws (B, 4), snr_db (B,) -> fp32 (noisy, clean), (B, leads, L)"""
    bank, noise = np.asarray(bank, dtype=np.float32), np.asarray(noise, dtype=np.float32)
    B = len(draws)
    noisy = np.empty((B, bank.shape[1], L), dtype=np.float32)
    clean = np.empty_like(noisy)
    for i, (row, start, kind, offset) in enumerate(np.asarray(draws).tolist()):
        x = bank[row, :, start:start + L].astype(np.float64)
        n = noise[kind, :, offset:offset + L].astype(np.float64)
        d = x - x.mean(axis=1, keepdims=True)
        std = np.sqrt((d * d).mean(axis=1, keepdims=True))
        c = d / np.maximum(std, 1e-6)
        pc, pn = (c * c).sum(), (n * n).sum()
        scale = np.sqrt(pc / 10.0 ** (float(snr_db[i]) / 10.0) / pn) if pn != 0.0 else 0.0
        clean[i] = c.astype(np.float32)
        noisy[i] = (c + scale * n).astype(np.float32)
    return noisy, clean


def ulp_distance(a, b):
    """fp32 arrays -> the largest distance in units in the last place (finite values; +0 and -0 are 0 apart)"""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max())


def make_case(N, leads, Lsrc, K, Tn, seed):
    """a seeded clean bank with per-lead offsets and gains (ADC-like, so the z-score has work to do) and K noise records"""
    rng = np.random.default_rng(seed)
    bank = (rng.standard_normal((N, leads, Lsrc)) * rng.uniform(0.5, 200.0, (N, leads, 1))
            + rng.uniform(-1000.0, 1000.0, (N, leads, 1))).astype(np.float32)
    noise = (rng.standard_normal((K, leads, Tn)) * rng.uniform(0.1, 50.0, (K, leads, 1))).astype(np.float32)
    return bank, noise
