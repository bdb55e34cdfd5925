"""Sample-rate conversion, host side (no GPU): the definition against scipy's recorded results, the frontier and length
formulas against brute force, the pool's planning over random chunkings, the refusals."""
import os
from fractions import Fraction

import numpy as np
import pytest

import rate_util as U
from ecg_denoise_amd import RalError, _lib, rate

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_rate.npz")
ALL_PAIRS = [(fs, 360) for fs in U.RATES] + [(360, fs) for fs in U.RATES]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("fs_in,fs_out", U.PAIRS)
def test_restatement_and_bank_match_scipy(fs_in, fs_out, golden):
    up, down = rate.rate_ratio(fs_in, fs_out)
    assert (up, down) == U.ratio(fs_in, fs_out)
    half = 10 * max(up, down)
    want = golden[f"bank_{fs_in}_{fs_out}"]
    for h in (rate.rate_bank(up, down), U.bank(up, down)):
        assert h.dtype == np.float64 and h.shape == (2 * half + 1,)
        assert np.max(np.abs(h[:half + 1] - want)) <= 1e-14 * np.max(np.abs(want))
        assert np.max(np.abs(h - h[::-1])) <= 1e-14 * np.max(np.abs(want))      # the fixture keeps one half: the other mirrors it
    for T in U.LENGTHS[(fs_in, fs_out)]:
        x, y = golden[f"x_{fs_in}_{fs_out}_{T}"].astype(np.float64), golden[f"y_{fs_in}_{fs_out}_{T}"]
        assert y.shape[-1] == rate.rate_length(T, up, down) == U.length(T, up, down)
        got = U.convert(x, up, down, rate.rate_bank(up, down))
        err = np.max(np.abs(got - y)) / np.max(np.abs(x))
        print(f"{fs_in}->{fs_out} T={T}: restatement vs scipy {err:.1e} of max|x|")
        assert err <= 1e-12


@pytest.mark.parametrize("fs_in,fs_out", ALL_PAIRS)
def test_frontier_and_length_against_brute_force(fs_in, fs_out):
    up, down = rate.rate_ratio(fs_in, fs_out)
    rate.rate_check(up, down)                     # every listed pair fits the kernel
    half = 10 * max(up, down)
    assert rate.rate_half(up, down) == half
    assert rate.rate_latency(fs_in, fs_out) == half / up
    m_max = (3 * half * up) // down + 2
    q = np.arange(m_max + 1) * down
    for n in range(3 * half + 1):
        final = q + half < n * up                 # output m is final iff its newest tap lies before sample n
        assert not final[-1]
        assert rate.rate_frontier(n, up, down) == int(np.argmin(final)), n      # the first m that is not final
        exist = q < n * up                        # output m exists iff its instant m down / up lies before the end
        assert rate.rate_length(n, up, down) == int(np.argmin(exist)), n
        assert rate.rate_frontier(n, up, down) <= rate.rate_length(n, up, down)


def _oldest_sample(m, up, down):
    """the oldest sample the kernel reads for output m: its K taps end at floor((m down + half) / up)"""
    half = 10 * max(up, down)
    return (m * down + half) // up - (rate.rate_taps_per_output(up, down) - 1)


@pytest.mark.parametrize("fs_in,fs_out", [(500, 360), (360, 500), (257, 360), (360, 128), (1000, 360), (360, 360)])
def test_pool_plan_over_random_chunkings(fs_in, fs_out):
    up, down = rate.rate_ratio(fs_in, fs_out)
    rng = np.random.default_rng(fs_in + 7 * fs_out)
    st = rate.RatePoolState(up, down, leads=2, capacity=3)
    assert st.hist_len == (2 * 10 * max(up, down)) // up + 1
    for trial in range(6):
        sids = [st.open() for _ in range(3)]
        T = {sid: int(rng.integers(1, 4000)) for sid in sids}
        got = {sid: 0 for sid in sids}
        while sids:
            shapes, close = {}, []
            for sid in sids:
                if rng.random() < 0.3:
                    continue                       # this call omits the stream
                left = T[sid] - int(st.n[sid])
                c = min(left, int(rng.choice([0, 1, 1, 2, 17, 300, 2500])))
                if c == left and rng.random() < 0.5:
                    close.append(sid)              # a close with a last chunk, or (c == 0) without one
                if c or sid not in close or rng.random() < 0.5:
                    shapes[sid] = (2, c)
            if not shapes and not close:
                continue
            before = (st.n.copy(), st.turn.copy(), st.is_open.copy(), list(st.free))
            order, tab = st.plan(shapes, close)
            assert all(np.array_equal(a, b) for a, b in zip(before, (st.n, st.turn, st.is_open, st.free)))   # plan changes nothing
            assert list(tab["x_off"]) == list(np.cumsum(tab["c"]) - tab["c"])
            assert list(tab["out_off"]) == list(np.cumsum(tab["m"]) - tab["m"])
            for sid, t in zip(order, tab):
                n1 = int(t["n0"] + t["c"])
                assert t["slot"] == sid and t["m0"] == got[sid] == st.frontier(t["n0"]) and t["m"] >= 0
                if sid in close:
                    assert t["T"] == n1 == T[sid] and t["flags"] == 0
                    assert t["m0"] + t["m"] == st.length(T[sid])
                else:
                    assert t["T"] == -1 and t["flags"] == _lib.POOL_KEEP
                    assert t["m0"] + t["m"] == st.frontier(n1)
                if t["m"] and not st.identity:     # the first output's oldest sample lies inside the history (or is clamped to 0)
                    assert max(_oldest_sample(int(t["m0"]), up, down), 0) >= t["n0"] - st.hist_len
                got[sid] += int(t["m"])
            turn = st.turn.copy()
            st.commit(tab)
            for sid, t in zip(order, tab):
                assert st.turn[sid] == (turn[sid] ^ 1 if sid not in close and not st.identity else turn[sid])
                if sid in close:
                    assert got[sid] == st.length(T[sid]) and not st.is_open[sid]
                    sids.remove(sid)
                else:
                    assert st.n[sid] == t["n0"] + t["c"]


def test_refusals():
    for bad in (499.5, 0, -360, "500", True, None, float("nan"), Fraction(0)):
        with pytest.raises(RalError):
            rate.rate_ratio(bad, 360)
        with pytest.raises(RalError):
            rate.rate_ratio(360, bad)
    assert rate.rate_ratio(500.0, 360) == (18, 25)                              # an integral float is an integer
    assert rate.rate_ratio(Fraction(1000, 3), 360) == (27, 25)
    for up, down in ((1, 360), (1021, 1024), (4001, 4000), (7, 100000)):           # banks or spans beyond the LDS budget
        with pytest.raises(RalError, match=f"up={up} down={down}"):
            rate.rate_check(up, down)
        with pytest.raises(RalError, match=f"up={up} down={down}"):
            rate.RatePoolState(up, down, 2, 4)
    st = rate.RatePoolState(18, 25, leads=2, capacity=2)
    a = st.open()
    with pytest.raises(RalError, match="not an open stream"):
        st.plan({a + 1: (2, 10)})
    with pytest.raises(RalError, match="not an open stream"):
        st.plan({"a": (2, 10)})
    with pytest.raises(RalError, match="not an open stream"):
        st.plan({}, close=(7,))
    with pytest.raises(RalError, match=r"expected a chunk of shape \(2, samples\)"):
        st.plan({a: (12, 10)})
    with pytest.raises(RalError, match=r"expected a chunk of shape \(2, samples\)"):
        st.plan({a: (10,)})
    with pytest.raises(RalError, match="without a single sample"):
        st.plan({}, close=(a,))
    with pytest.raises(RalError, match="nothing to do"):
        st.plan({})
    b = st.open()
    with pytest.raises(RalError, match="all 2 slots"):
        st.open()
    assert (a, b) == (0, 1) and st.n.sum() == 0 and st.is_open.all()
