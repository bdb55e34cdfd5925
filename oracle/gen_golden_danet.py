"""Golden fixture of the DANet baseline (build container only; imports the REFERENCE's model/DAM.py from /root/reference).

  tests/golden/g3_danet_L512.npz   Seq2Seq2 (DAM.py:341-349) at (6, 2, 512) with the build-owned state of
                                   oracle/danet_oracle.init_state(4321): train-mode output, MSE loss, every parameter
                                   gradient (summaries for the large ones), running statistics after the step, eval-mode
                                   output from the INITIAL state.
  tests/golden/g3_danet_ties_L256.npz   Seq2Seq2 in float64 at (8, 2, 256) on tests/tie_util.danet_tie_batch (every even
                                   window one 32-sample beat repeated, so that nn.AdaptiveMaxPool1d(1) meets equal maxima)
                                   with tie_util.danet_negated_state (init_state(99), some DAM-cell BatchNorm gains
                                   negated): train-mode output, MSE loss, every parameter gradient, the input gradient.

    python oracle/gen_golden_danet.py          (both)
    python oracle/gen_golden_danet.py ties     (the second alone)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")
import danet_oracle as D  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(2)
    from model.DAM import Seq2Seq2
    m = Seq2Seq2()
    B, L = 6, 512
    gg = torch.Generator().manual_seed(2023)
    x = torch.randn(B, 2, L, generator=gg); tgt = torch.randn(B, 2, L, generator=gg)
    m.train()
    with torch.no_grad():
        m(x)                                    # materialise the Lazy modules
    st = D.init_state(4321)
    assert list(m.state_dict().keys()) == list(st.keys()), "state_dict order"
    m.load_state_dict(st)
    m.eval()
    with torch.no_grad():
        y_eval = m(x).numpy().copy()
    m.train()
    y = m(x)
    loss = torch.nn.functional.mse_loss(y, tgt)
    loss.backward()
    out = {"x": x.numpy(), "target": tgt.numpy(), "y_eval": y_eval, "y_train": y.detach().numpy(), "loss": np.float64(loss.item())}
    for k, p in m.named_parameters():
        out["grad_" + k] = p.grad.numpy()
    sd = m.state_dict()
    for k in sd:
        if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked"):
            out["after_" + k] = sd[k].numpy().copy()
    np.savez_compressed(os.path.join(OUT, "g3_danet_L512.npz"), **out)
    print("g3_danet_L512: loss", loss.item(), "keys", len(out), "params", sum(p.numel() for p in m.parameters()))


def ties():
    """the reference in float64 where its max-pools have to choose: tests/tie_util.py's periodic batch at (8, 2, 256) and its
    state with negated BatchNorm gains"""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import tie_util as T
    from model.DAM import Seq2Seq2
    torch.manual_seed(0)
    torch.set_num_threads(1)
    L, period, B = T.DANET_CASES[0]
    x, tgt = T.danet_tie_batch(L, period, B)
    m = Seq2Seq2()
    m.train()
    with torch.no_grad():
        m(x)                                    # materialise the Lazy modules
    m.double()
    st = T.danet_negated_state(torch.float64)
    assert list(m.state_dict().keys()) == list(st.keys()), "state_dict order"
    m.load_state_dict(st)
    xd = x.double().requires_grad_(True)
    y = m(xd)
    loss = torch.nn.functional.mse_loss(y, tgt.double())
    loss.backward()
    out = {"x": xd.detach().numpy(), "target": tgt.double().numpy(), "y_train": y.detach().numpy(), "loss": np.float64(loss.item()),
           "dx": xd.grad.numpy()}
    for k, p in m.named_parameters():
        out["grad_" + k] = p.grad.numpy()
    assert all(v.dtype == np.float64 for v in out.values())
    # torch's CPU convolution keeps a periodic window bit-periodic on some hosts only (tie_util.conv1d_by_taps): where it does
    # not, the reference has no ties to choose between and this is no fixture
    e = T.per_window(out["dx"], T.danet_oracle_step(st, x, tgt)["dx"].numpy())
    assert e.max() < 1e-9, ("on this host the reference's convolutions are not position-independent", e)
    np.savez_compressed(os.path.join(OUT, "g3_danet_ties_L256.npz"), **out)
    print("g3_danet_ties_L256: loss", loss.item(), "keys", len(out))


if __name__ == "__main__":
    if sys.argv[1:] != ["ties"]:
        main()
    if sys.argv[1:] in ([], ["ties"]):
        ties()
