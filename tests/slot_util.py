"""What the GPU tests of the pools with a raw-sample history (`ResamplerPool`, `BeatPool`) share: a run that asserts the
history planes themselves, as the slot protocol (csrc/ral_slots.hpp) states them."""
import torch


def expected_history(rec, n, hist_len):
    """the last hist_len of the first n samples of rec (leads, T), zeros where the stream has fewer"""
    want = torch.zeros(rec.shape[0], hist_len, dtype=rec.dtype, device=rec.device)
    have = min(n, hist_len)
    want[:, hist_len - have:] = rec[:, n - have:n]
    return want


def run_with_history_checks(pool, recs):
    """recs: four device records (leads, T) for a pool of capacity 3: records 0 and 2 longer than 3 hist_len + 1 samples, record
    1 of exactly that length, record 3 longer than hist_len + 3.  Streams 0 .. 2 are pushed from their first sample in chunks
    of 1, hist_len - 1, hist_len and hist_len + 1 samples (each stream at another place of that cycle); stream 1 ends there,
    both planes of its slot are overwritten with NaN, and stream 3 opens in that slot and is pushed sample by sample for
    hist_len + 3 samples.  After every
    push the current plane of every open stream must hold the last hist_len samples received, zeros below sample 0 (so never a
    NaN).  Then the streams are closed with the rest of their records.  -> per stream the list of its results, in order."""
    hl = pool.hist_len
    lens = [1, hl - 1, hl, hl + 1]
    sid, pos, outs = {}, {}, {i: [] for i in range(4)}

    def push(which, take):
        chunks = {sid[i]: recs[i][:, pos[i]:pos[i] + take[i]] for i in which}
        res = pool.push(chunks)
        for i in which:
            pos[i] += take[i]
            outs[i].append(res[sid[i]])
        for i in sid:
            slot = sid[i]
            assert pool.samples_in(slot) == pos[i]
            got = pool.hist[int(pool.state.turn[slot]), slot]
            assert torch.equal(got, expected_history(recs[i], pos[i], hl)), (i, pos[i])

    for i in range(3):
        sid[i], pos[i] = pool.open(), 0
    for k in range(4):
        push((0, 1, 2), {i: lens[(k + i) % 4] for i in range(3)})
    assert pos[1] == 3 * hl + 1 == recs[1].shape[1]
    old = sid.pop(1)
    outs[1].append(pool.close(old))
    pool.hist[:, old].fill_(float("nan"))
    sid[3], pos[3] = pool.open(), 0
    assert sid[3] == old
    for _ in range(hl + 3):
        push((3,), {3: 1})
    for i in sid:
        outs[i].append(pool.close(sid[i], recs[i][:, pos[i]:]))
    assert pool.open_streams == ()
    return [outs[i] for i in range(4)]
