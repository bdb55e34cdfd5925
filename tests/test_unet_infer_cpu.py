"""The premises of tests/test_gpu_unet_infer.py, checked without a device: the batches wrap the fused kernel's persistent grid
whatever its occupancy, the windows compared bit for bit lie in a workgroup's first, second and third round, the warmed
BatchNorm statistics are away from their defaults, the outputs are signal and not a per-lead constant, and the 1e-5 bar per
window has headroom over fp32 arithmetic itself.

Here (256 CUs; leads 1 / 2):
  L      LDS bytes  bound  wrap batch   signal share, least   fp32 oracle against fp64, worst window
  256    29856      1280   2597         0.951 / 0.970         2.5e-7 / 2.9e-7
  512    55968      512    1061         0.976 / 0.984         2.1e-7 / 2.6e-7
  768    82080      256    549          0.986 / 0.989         2.1e-7 / 2.5e-7
  1024   108192     256    549          0.987 / 0.989         2.0e-7 / 2.4e-7
running means in -0.42 .. 0.78 (one lead) and -0.77 .. 0.61 (two), running variances in 0.046 .. 0.85.  Seeds as the defaults of
unet_infer_util (parameters 1234, data 7): no other seed was needed to meet the conditions."""
import numpy as np
import pytest

import ralenet_oracle as O
import unet_infer_util as U

CUS = 256
LDS_BYTES = {256: 29856, 512: 55968, 768: 82080, 1024: 108192}      # by hand from k_unet_infer's carve-up (tests/test_unet_plan_cpu.py)
WRAP = {256: 2597, 512: 1061, 768: 549, 1024: 549}


@pytest.mark.parametrize("leads,L", U.CASES)
def test_the_batch_wraps_every_workgroup(leads, L):
    name, threads, lds, fe = U.fused_plan(leads, L, 1)
    assert name == "k_unet_infer<%d>" % leads and threads == 256 and fe == 1 and lds == LDS_BYTES[L]
    bound, B = U.resident_bound(leads, L, CUS), U.wrap_batch(leads, L, CUS)
    assert bound == CUS * min(163840 // lds, 8) and B == WRAP[L]
    assert B > 2 * bound and B % bound != 0
    idx = U.pass_windows(B, CUS)
    assert idx == sorted(set(idx)) and idx[0] == 0 and idx[-1] == B - 1
    assert {0, 1, CUS - 1, CUS, CUS + 1, 2 * CUS - 1, 2 * CUS, B - 38, B - 37, B - 1} <= set(idx)
    for m in range(3 * CUS, B, CUS):
        assert {m - 1, m} <= set(idx) and (m + 1 >= B or m + 1 in idx)
    for lo, hi in ((0, bound), (bound, 2 * bound), (2 * bound, B)):
        assert any(lo <= i < hi for i in idx), (lo, hi)
    # a device with other CU counts: the same properties
    for cus in (64, 228, 304):
        b2, B2 = U.resident_bound(leads, L, cus), U.wrap_batch(leads, L, cus)
        i2 = U.pass_windows(B2, cus)
        assert B2 > 2 * b2 and B2 % b2 != 0 and all(any(lo <= i < hi for i in i2) for lo, hi in ((0, b2), (b2, 2 * b2), (2 * b2, B2)))


@pytest.mark.parametrize("leads,L", U.CASES)
def test_the_warmed_state_and_the_inputs_make_the_bar_mean_something(leads, L):
    p32, bn = U.warmed_state(leads, L)
    for k in O.UNET_BN:
        mean, var = bn[k]["running_mean"].numpy(), bn[k]["running_var"].numpy()
        assert np.abs(mean).max() > 0.05, (k, mean)
        assert ((var < 0.8) | (var > 1.2)).any(), (k, var)
    sd = U.flat_state_dict(p32, bn)
    assert all(k + "." + s in sd for k in O.UNET_BN for s in ("running_mean", "running_var")) and all(k in sd for k in p32)
    B = U.wrap_batch(leads, L, CUS)
    x, ref = U.case_reference(leads, L, B)
    assert x.shape == (B, leads, L) and ref.dtype.is_floating_point and ref.element_size() == 8
    share = U.signal_share(ref)
    e32 = U.window_errors(U.oracle_eval(leads, L, x, dtype=x.dtype), ref)
    lo, hi, vlo, vhi = U.stats_range(bn)
    print(f"[unet infer] leads {leads} L {L} B {B}: running means {lo:.3f} .. {hi:.3f}, variances {vlo:.3f} .. {vhi:.3f}; signal share >= "
          f"{share.min():.3f} (window {share.argmin()}); fp32 oracle against fp64: worst window {e32.max():.2e} ({e32.argmax()})")
    assert share.min() >= 0.9, (share.min(), share.argmin())
    assert e32.max() < 1e-6, (e32.max(), e32.argmax())
