"""Entry and exit of every handle on a stream of the caller's (`pytest -m gpu`): the four networks of tests/test_gpu_handles.py at
its smallest shapes, RA-LENet at 128 windows on two lanes with side streams, and NewRALE around its frozen inner model run
two train steps and an eval forward on a stream S behind a bounded stall (tests/stall_util.py) and once more eagerly with a
device synchronisation after every call.

Behind the stall x, the target, the parameters, the BatchNorm state and the Adam moments are NaN until copies on S fill them;
the prediction, loss, SNR and RMSE of the first step, the loss of the second and the eval output are cloned on S right after
the call that produces them; x and the target are poisoned on S as soon as the last call is enqueued; only S is ever
synchronised.  A kernel on a stream that does not wait for S reads NaN or poisoned input, one that S does not wait for leaves a
clone incomplete - across the optimiser step too (`sums_clean`: the Adam kernel clears the BatchNorm sums of the next stem;
the reset of `dw_pending` between passes; the preparation stream after an Adam step; the adapter's `k_conv13_*` and
`ral_adam_flat`).

Bars: everything up to the first backward (first prediction, loss, SNR, RMSE) bit for bit.  The second step's loss and the final
eval output have passed an optimiser step, whose gradients carry float atomics: their bar is 8 times (parity_bars.K_PAIR, the project's largest factor) the difference
between two synchronised runs, floored at 1e-7 relative L2 and never above the forward bar 1e-5.

The negative control runs `ral_loss_means` on streams that do not wait for S and must see the NaN.

Seen on the MI355X (one run; every case reported `pending` True and every first-step quantity was the same bits in all three
runs).  enq: wall-clock time of the host to enqueue the body; stall: asked / achieved; body: gate -> end of the body on the device;
then, for the second step's loss and the final eval output, the relative L2 difference between the two synchronised runs (the
floor), the bar it gives, and the difference of the stalled run from the first synchronised one.

    network            enq ms  stall ms     body ms  loss2: floor   bar      stalled   eval: floor   bar      stalled
    ralenet             2.88   20.0 / 20.0   4.22    0              1.0e-7   0         2.95e-7       2.36e-6  3.19e-7
    unet                0.35   20.0 / 20.0   0.66    0              1.0e-7   0         0             1.0e-7   0
    acdae               0.34   20.0 / 19.9   0.68    0              1.0e-7   0         0             1.0e-7   0
    danet               0.96   20.0 / 20.0   1.13    0              1.0e-7   0         0             1.0e-7   0
    ralenet_two_lanes   3.22   20.0 / 19.9   5.88    7.86e-10       1.0e-7   3.15e-9   3.39e-7       2.71e-6  3.41e-7
    newrale             1.64   20.0 / 20.0   4.18    0              1.0e-7   0         0             1.0e-7   0

Negative control: stall 20.0 ms asked, 19.9 achieved; the call on S gave finite means, the calls on the four other streams NaN,
NaN, NaN and finite means (the fourth stream shared S's hardware queue and so ran behind the copy after all).
"""
import ctypes as C

import pytest
import torch

import schedule_util as S
import stall_util as U
from parity_bars import K_PAIR
from test_gpu_handles import B, DEV, NETWORKS

pytestmark = pytest.mark.gpu

FLOOR, FORWARD_BAR = 1e-7, 1e-5
CASES = list(NETWORKS) + ["ralenet_two_lanes", "newrale"]


def _build(net):
    """-> (model, x0, target0) at the smallest shape of tests/test_gpu_handles.py, or the two cases added here"""
    from ecg_denoise_amd import ACDAE, DANet, NewRALE, RALENet, UNet
    nb, leads, L = B, None, None
    if net == "ralenet_two_lanes":
        nb, leads, L = 128, 1, 256
        m = RALENet("full", leads=1, L=L, max_batch=nb, device=DEV, seed=7)
        S.rwave_tables(m, 4)
        S.set_schedule(m, 2, 1)
    elif net == "newrale":
        leads, L = 12, 256
        inner = RALENet("full", leads=2, L=L, max_batch=nb, device=DEV, seed=7)
        S.rwave_tables(inner, 4)
        m = NewRALE(inner, seed=8)
    else:
        variant, leads, L = NETWORKS[net]
        m = {"ralenet": lambda: RALENet(variant, leads=leads, L=L, max_batch=nb, device=DEV, seed=7),
             "unet": lambda: UNet(leads=leads, L=L, max_batch=nb, device=DEV, seed=7),
             "acdae": lambda: ACDAE(L=L, max_batch=nb, device=DEV, seed=7),
             "danet": lambda: DANet(L=L, max_batch=nb, device=DEV, seed=7)}[net]()
    g = torch.Generator().manual_seed(11)
    return m, torch.randn(nb, leads, L, generator=g).to(DEV), torch.randn(nb, leads, L, generator=g).to(DEV)


def _buffers(m):
    """every device buffer a train step reads and writes across calls: [(buffer, its initial value)]"""
    engines = [m.rale.eng] if hasattr(m, "rale") else [m.eng]
    bufs = [m.params, m.adam_m, m.adam_v] if hasattr(m, "rale") else []
    for e in engines:
        bufs += [e.params, e.state, e.adam_m, e.adam_v, e.bn_sums]
    return [(b, b.clone()) for b in bufs if b is not None and b.numel() > 0]


def _relerr(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("net", CASES)
def test_two_train_steps_and_an_eval_forward_behind_the_stall(net):
    St = torch.cuda.Stream()
    with torch.cuda.stream(St):
        m, x0, t0 = _build(net)
        m.train()
        bufs = _buffers(m)
        x, t = torch.empty_like(x0), torch.empty_like(t0)
    St.synchronize()
    inner = m.rale if hasattr(m, "rale") else m

    def before():
        for b in [x, t] + [b for b, _ in bufs]:
            U.poison(b)

    def body(sync=None):
        eager, sync = sync is not None, sync or (lambda: None)
        U.late(x, x0); U.late(t, t0)
        for b, v in bufs:
            U.late(b, v)
        m.step_count = 0
        inner._params_changed()
        m.train()
        sync()
        out = {}
        for k in (1, 2):
            if not eager:
                r = m.train_step(x, t)
            else:                                                  # train_step, call by call, the device synchronised after each
                if hasattr(m, "rale"):
                    pred = m.forward(x); sync()
                    loss, snr, rmse = m.loss_and_metrics(pred, t); sync()
                else:
                    pred, loss, snr, rmse = m.forward_loss(x, t); sync()
                m.backward(); sync()
                m.step(1e-3); sync()
                r = {"loss": loss, "pred": pred, "snr": snr, "rmse": rmse}
            if k == 1:
                out.update({n: r[n].clone() for n in ("pred", "loss", "snr", "rmse")})
            else:
                out["loss2"] = r["loss"].clone()
        m.eval()
        out["eval"] = m(x).clone()
        sync()
        m.train()
        U.poison(x); U.poison(t)
        sync()
        return out

    refs = []
    for _ in range(2):                                             # eagerly, on the default stream
        before(); torch.cuda.synchronize()
        refs.append(body(torch.cuda.synchronize))
    torch.cuda.synchronize()
    got, st, _ = U.run_stalled(St, body, f"handle {net}", before)
    assert st.pending is True
    for tag, res in (("synchronised", refs[0]), ("synchronised again", refs[1]), ("stalled", got)):
        for k, v in res.items():
            assert torch.isfinite(v).all(), (tag, k)
    for k in ("pred", "loss", "snr", "rmse"):
        assert torch.equal(refs[1][k], refs[0][k]), ("the synchronised step run twice", k)
        assert torch.equal(got[k], refs[0][k]), k
    line, bad = [], {}
    for k in ("loss2", "eval"):
        floor = _relerr(refs[1][k], refs[0][k])
        bar = min(max(K_PAIR * floor, FLOOR), FORWARD_BAR)
        err = _relerr(got[k], refs[0][k])
        line.append(f"{k}: synchronised runs differ by {floor:.2e}, bar {bar:.2e}, stalled run differs by {err:.2e}")
        if not err <= bar:
            bad[k] = (err, bar)
    print(f"[stall] handle {net}: " + "; ".join(line))
    assert not bad, bad
    assert not torch.equal(got["eval"], got["pred"])               # (the optimiser steps moved the model)


def test_a_call_on_a_stream_that_ignores_the_callers_is_seen():
    """The negative control, on `ral_loss_means` alone (5 x 1024; NaN in a loss kernel is a supported input): `pred` is NaN
    until a copy on S behind the stall fills it; the same call on S gives finite means, on a stream that does not wait for S
    means with NaN in them.  Streams share hardware queues, and a queue runs its packets in order: a second stream that happens
    to share S's queue waits for S after all, so the call goes to four fresh streams, each with buffers of its own, and
    at least one of them must show the NaN."""
    from ecg_denoise_amd import _lib
    n, rows = 1024, 5
    St = torch.cuda.Stream()
    others = [torch.cuda.Stream() for _ in range(4)]
    g = torch.Generator().manual_seed(5)
    good, target = torch.randn(rows, n, generator=g).to(DEV), torch.randn(rows, n, generator=g).to(DEV)
    pred = torch.empty_like(good)
    out = [{"snr": torch.zeros(rows, device=DEV), "rmse": torch.zeros(rows, device=DEV), "means": torch.zeros(3, dtype=torch.float64, device=DEV),
            "scratch": torch.zeros(64, dtype=torch.float64, device=DEV)} for _ in range(1 + len(others))]
    p = lambda v: C.c_void_p(v.data_ptr())

    def call(o, stream):
        _lib.check(_lib.lib().ral_loss_means(p(pred), p(target), n, rows, rows, C.c_void_p(0), p(o["snr"]), p(o["rmse"]), p(o["means"]),
                                             p(o["scratch"]), C.c_void_p(stream.cuda_stream)))

    call(out[0], St)                                               # (warm: the kernel's code is loaded before the stall)
    with torch.cuda.stream(St):
        U.poison(pred)
    torch.cuda.synchronize()
    with U.stalled(St, U.STALL_FLOOR_MS) as st:
        U.late(pred, good)
        call(out[0], St)
        for o, s in zip(out[1:], others):
            call(o, s)
    st.premise("negative control")
    St.synchronize()
    for s in others:
        s.synchronize()
    seen = [bool(torch.isnan(o["means"]).any().item()) for o in out]
    print(f"[stall] negative control: stall asked {st.ms:.1f} ms, achieved {st.achieved_ms():.1f} ms; NaN in the means of the call on S {seen[0]}, "
          f"on four streams that do not wait for S {seen[1:]}")
    assert seen[0] is False and torch.isfinite(out[0]["means"]).all()
    assert any(seen[1:]), seen
