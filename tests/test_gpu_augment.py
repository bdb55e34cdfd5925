"""ral_mix_batch / NoiseMixSampler on the device against the NumPy restatement (tests/augment_util.py): the draws exactly, the
mixed windows to one fp32 unit in the last place; independence of batch size and shard; training through `train()`."""
import numpy as np
import pytest
import torch

from augment_util import draw_ref, make_case, mix_ref, ulp_distance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SNR = (-4.0, 30.0)


def _sampler(bank, noise, L, **kw):
    from ecg_denoise_amd import NoiseMixSampler
    args = dict(L=L, snr_db=SNR, seed=2023, device=DEV)
    args.update(kw)
    return NoiseMixSampler(bank, noise, **args)


def _fields(b):
    """a MixedBatch as host arrays, in a fixed order"""
    return [getattr(b, k).cpu().numpy() for k in ("noisy", "clean", "row", "start", "kind", "offset", "snr_db")]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_against_restatement(s, b, bank, noise, B, first, rows=None):
    noisy, clean, row, start, kind, offset, snr = _fields(b)
    want, wsnr = draw_ref(s.seed, first, B, s.N, s.Lsrc, s.L, s.Tn, s.thresholds, *s.snr_db)
    if rows is not None:
        want[:, 0] = rows
    got = np.stack([row, start, kind, offset], axis=1).astype(np.int64)
    assert np.array_equal(got, want), (got, want)
    assert np.abs(snr - wsnr).max() <= 1e-12
    rn, rc = mix_ref(bank, noise, got, snr, s.L)                       # the restatement mixes at the RETURNED snr_db
    assert noisy.shape == clean.shape == (B, s.leads, s.L) and np.isfinite(noisy).all() and np.isfinite(clean).all()
    uc, un = ulp_distance(clean, rc), ulp_distance(noisy, rn)
    print(f"B={B} leads={s.leads} L={s.L}: clean {uc} ulp, noisy {un} ulp from the restatement")
    assert uc <= 1 and un <= 1, (uc, un)


# (B, leads, L, Lsrc, N, K, Tn, first)
CASES = [
    (1, 1, 16, 16, 1, 1, 16, 0),                # every range is a single value; fewer samples than lanes
    (5, 2, 48, 200, 7, 3, 1000, 0),             # L not a multiple of 64; B not a multiple of anything
    (3, 12, 1024, 1024, 4, 2, 1500, 0),         # the largest footprint the models use
    (2, 16, 64, 80, 3, 8, 64, 0),               # maximum leads and K; one possible offset
    (8, 2, 64, 64, 5, 3, 300, 2 ** 32 - 3),     # the high counter word changes inside the call
    (4, 2, 50, 70, 3, 2, 200, 0),               # L not a multiple of 4: the element pass one sample per lane; pieces of 25
    (3, 3, 36, 40, 2, 2, 90, 0),                # three leads: one piece per lead, a wave without work
]


@pytest.mark.parametrize("B,leads,L,Lsrc,N,K,Tn,first", CASES)
def test_batch_matches_the_restatement(B, leads, L, Lsrc, N, K, Tn, first):
    bank, noise = make_case(N, leads, Lsrc, K, Tn, seed=B + leads)
    s = _sampler(bank, noise, L, weights=tuple(range(1, K + 1)))
    s.position = first
    b = s.batch(B)
    assert b.first == first and s.position == (first + B) % 2 ** 64
    _check_against_restatement(s, b, bank, noise, B, first)


def test_rows_override_is_used_verbatim_and_changes_nothing_else():
    bank, noise = make_case(9, 2, 120, 3, 700, seed=11)
    s, t = _sampler(bank, noise, 96), _sampler(bank, noise, 96)
    rows = torch.tensor([8, 0, 3, 3, 5, 1, 7], device=DEV)
    a, b = s.batch(7), t.batch(7, rows=rows)
    fa, fb = _fields(a), _fields(b)
    assert np.array_equal(fb[2], rows.cpu().numpy()) and not np.array_equal(fa[2], fb[2])
    assert _same(fa[3:], fb[3:])                                        # start, kind, offset, snr_db: as without rows
    _check_against_restatement(t, b, bank, noise, 7, 0, rows=rows.cpu().numpy())
    # a row outside the bank reads nothing: that window is NaN, its row -1, the others as before
    bad = rows.clone(); bad[2] = 9
    u = _sampler(bank, noise, 96)
    fc = _fields(u.batch(7, rows=bad))
    assert fc[2][2] == -1 and np.isnan(fc[0][2]).all() and np.isnan(fc[1][2]).all()
    keep = [0, 1, 3, 4, 5, 6]
    assert all(np.array_equal(x[keep], y[keep]) for x, y in zip(fb, fc))


def test_degenerate_inputs():
    bank, noise = make_case(2, 2, 64, 2, 64, seed=13)                  # Lsrc == L and Tn == L: start 0 and offset 0
    bank[:, 0] = -3.25                                                 # a constant lead in every row
    noise[1] = 0.0                                                     # an all-zero noise kind
    s = _sampler(bank, noise, 64)
    noisy, clean, row, start, kind, offset, snr = _fields(s.batch(16))
    assert set(kind.tolist()) == {0, 1}
    assert np.isfinite(noisy).all() and np.isfinite(clean).all()
    assert (clean[:, 0] == 0).all() and (clean[:, 1] != 0).any()
    z = kind == 1
    assert np.array_equal(noisy[z].view(np.int32), clean[z].view(np.int32))      # bit for bit
    assert not np.array_equal(noisy[~z], clean[~z])


def test_achieved_snr():
    """10 log10(sum clean^2 / sum (noisy - clean)^2) of the fp32 outputs against the returned snr_db.  The restatement's own
    fp32-rounded outputs, at this shape and these draws (64 windows of 2 x 256, snr_db drawn in [-4, 30) dB, -3.6 .. 28.2 dB
    drawn), miss the asked SNR by at most 9.1e-7 dB (measured on the CPU; the worst window is one near +28 dB, where the fp32
    rounding of noisy and clean is largest against the noise); 4x that for summation order and the device's pow."""
    bank, noise = make_case(20, 2, 300, 3, 2000, seed=17)
    s = _sampler(bank, noise, 256)
    noisy, clean, *_, snr = _fields(s.batch(64))
    assert snr.min() < 0 and snr.max() > 28
    c = clean.astype(np.float64)
    e = noisy.astype(np.float64) - c
    got = 10 * np.log10((c * c).sum((1, 2)) / (e * e).sum((1, 2)))
    print(f"achieved SNR: worst miss {np.abs(got - snr).max():.3e} dB")
    assert np.abs(got - snr).max() <= 4 * 9.1e-7


def test_independent_of_batch_size_and_shard():
    bank, noise = make_case(9, 2, 120, 3, 700, seed=19)
    cat = lambda *bs: [np.concatenate(f) for f in zip(*(_fields(b) for b in bs))]
    one = _sampler(bank, noise, 96)
    whole = _fields(one.batch(10))
    nxt = _fields(one.batch(10))
    assert not any(np.array_equal(x, y) for x, y in zip(whole, nxt))    # two consecutive batches differ in every field
    two = _sampler(bank, noise, 96)
    assert _same(cat(two.batch(6), two.batch(4)), whole)
    r0, r1 = _sampler(bank, noise, 96, rank=0, world=2), _sampler(bank, noise, 96, rank=1, world=2)
    assert _same(cat(r0.batch(5), r1.batch(5)), whole)
    assert _same(cat(r0.batch(5), r1.batch(5)), nxt) and r0.position == r1.position == one.position == 20
    state = one.state_dict()
    third = _fields(one.batch(10))
    resumed = _sampler(bank, noise, 96, seed=1)
    resumed.load_state_dict(state)
    assert _same(_fields(resumed.batch(10)), third)


def test_training_through_train(tmp_path):
    from ecg_denoise_amd import UNet
    from ecg_denoise_amd.train import train
    bank, noise = make_case(12, 2, 100, 3, 500, seed=23)
    s = _sampler(bank, noise, 64, snr_db=(-4.0, 4.0))
    test_loader, train_loader = s.loader(2, 2, replay=True), s.loader(2, 3)
    first, second = [list(test_loader) for _ in range(2)]
    assert len(first) == 2 and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(first, second))
    assert not torch.equal(first[0][0], first[1][0])
    m = UNet(leads=2, L=64, max_batch=2, device=DEV, seed=5)
    losses, step = [], m.train_step
    def recording_step(x, t, lr):                                      # train() keeps only the epoch mean
        out = step(x, t, lr)
        losses.append(out["loss"].clone())
        return out
    m.train_step = recording_step
    res = train(1, m, 2, train_loader, test_loader, model_name="unet", noise_name="mixed", noise_intensity="m4p4",
                out_dir=str(tmp_path), log=lambda *a: None)
    assert len(losses) == 3 and s.position == 2 * 2 + 3 * 2
    assert all(np.isfinite(v[0]) for v in res) and all(np.isfinite(v[0]) for v in train.last_losses)
    # the same steps by hand, on the batches of a second sampler with the same seed
    s2 = _sampler(bank, noise, 64, snr_db=(-4.0, 4.0))
    s2.loader(2, 2, replay=True)                                       # sets the same four ordinals aside
    m2 = UNet(leads=2, L=64, max_batch=2, device=DEV, seed=5)
    m2.train()
    hand = []
    for _ in range(3):
        b = s2.batch(2)
        hand.append(m2.train_step(b.noisy, b.clean, 1e-3)["loss"].clone())
    got, want = torch.cat(losses).cpu().numpy(), torch.cat(hand).cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got.view(np.int64), want.view(np.int64)), (got, want)
