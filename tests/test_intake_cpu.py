"""`ecg_denoise_amd.intake`: the one reader of beat lists, under the settings of its four callers, on host tensors only.

One table of bad inputs says which caller refuses what, and in which words; one table of good inputs says that all four build
the same padded tensors.  The texts are the ones the callers raised while each had a reader of its own."""
import numpy as np
import pytest
import torch

from ecg_denoise_amd import Beats, RalError
from ecg_denoise_amd.intake import beat_lists, check_leads, pad_rows

CPU = torch.device("cpu")
T, R = 1000, 2
# what each caller passes: (what, keyword arguments)
CALLERS = {
    "match_beats": ("match_beats", dict(strict=False, name="ref")),
    "classify": ("BeatClassifier.classify", dict(T=T, R=R)),
    "delineate": ("BeatDelineator.delineate", dict(T=T, R=R)),
    "analyse": ("HrvAnalyzer.analyse", dict(T=T)),
}
STRICT = "{what}: the beats of a record must be strictly ascending positions in [0, 1000)"
LOOSE = "match_beats: ref must hold ascending sample indices in [0, 2^31)"


def _read(caller, beats):
    what, kw = CALLERS[caller]
    return beat_lists(beats, CPU, what, **kw)


def _wrong_beats():
    return Beats(torch.full((3, 4), -1, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))


# input -> {caller: the message, or None where the caller accepts it}
BAD = [
    ("descending", lambda: [[9, 3], [1]], dict(match_beats=LOOSE, classify=STRICT, delineate=STRICT, analyse=STRICT)),
    ("repeated", lambda: [[5, 5], [1]], dict(match_beats=None, classify=STRICT, delineate=STRICT, analyse=STRICT)),
    ("negative", lambda: [[-1], [1]], dict(match_beats=LOOSE, classify=STRICT, delineate=STRICT, analyse=STRICT)),
    ("at T", lambda: [[1], [1000]], dict(match_beats=None, classify=STRICT, delineate=STRICT, analyse=STRICT)),
    ("at 2^31", lambda: [[1], [2 ** 31]], dict(match_beats=LOOSE, classify=STRICT, delineate=STRICT, analyse=STRICT)),
    ("one list for two records", lambda: [[5]],
     dict(match_beats=None, classify="{what}: 1 beat lists for 2 records", delineate="{what}: 1 beat lists for 2 records", analyse=None)),
    ("three lists for two records", lambda: [[5], [6], [7]],
     dict(match_beats=None, classify="{what}: 3 beat lists for 2 records", delineate="{what}: 3 beat lists for 2 records", analyse=None)),
    ("no list at all", lambda: [],
     dict(match_beats="match_beats: ref holds no record", classify="{what}: 0 beat lists for 2 records",
          delineate="{what}: 0 beat lists for 2 records", analyse="{what}: no record")),
    ("a Beats of three records", _wrong_beats,
     dict(match_beats=None, classify="{what}: 3 beat lists on cpu for 2 records on cpu",
          delineate="{what}: 3 beat lists on cpu for 2 records on cpu", analyse=None)),
]


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_every_caller_refuses_what_it_refused_and_in_its_own_words(case):
    _, make, want = case
    assert set(want) == set(CALLERS)
    for caller, text in want.items():
        if text is None:
            peaks, count = _read(caller, make())
            assert peaks.dtype == count.dtype == torch.int32 and peaks.shape[0] == count.shape[0]
        else:
            with pytest.raises(RalError) as e:
                _read(caller, make())
            assert str(e.value) == text.format(what=CALLERS[caller][0]), caller


def test_match_beats_names_the_list_it_refuses():
    with pytest.raises(RalError, match=r"^match_beats: det must hold ascending sample indices in \[0, 2\^31\)$"):
        beat_lists([[3, 2]], CPU, "match_beats", strict=False, name="det")
    with pytest.raises(RalError, match=r"^match_beats: det holds no record$"):
        beat_lists([], CPU, "match_beats", strict=False, name="det")


GOOD = [
    [[3, 10, 999], []],
    [[], [0]],
    [[0, 1, 2, 3, 4], [7]],
    [np.array([5, 6], dtype=np.int16), torch.tensor([1, 500, 998])],
    [(4, 8), range(10, 20)],
]


@pytest.mark.parametrize("lists", GOOD)
def test_all_four_callers_build_the_same_tensors(lists):
    rows = [[int(v) for v in r] for r in lists]
    cap = max(1, max(len(r) for r in rows))
    want = torch.tensor([r + [-1] * (cap - len(r)) for r in rows], dtype=torch.int32)
    for caller in CALLERS:
        peaks, count = _read(caller, lists)
        assert peaks.dtype == torch.int32 and count.dtype == torch.int32 and peaks.is_contiguous()
        assert torch.equal(peaks, want) and count.tolist() == [len(r) for r in rows], caller
    b = Beats(want, torch.tensor([len(r) for r in rows], dtype=torch.int32))
    for caller in CALLERS:                                  # a Beats goes through as it is
        peaks, count = _read(caller, b)
        assert peaks.data_ptr() == b.peaks.data_ptr() and count.data_ptr() == b.count.data_ptr()


def test_a_beats_with_a_wider_cap_or_strided_storage_comes_out_contiguous_and_unchanged():
    wide = torch.full((2, 9), -1, dtype=torch.int32)
    wide[:, :2] = torch.tensor([[1, 2], [3, 4]], dtype=torch.int32)
    b = Beats(wide[:, ::2], torch.tensor([1, 1], dtype=torch.int32))
    for caller in CALLERS:
        peaks, count = _read(caller, b)
        assert peaks.is_contiguous() and torch.equal(peaks, wide[:, ::2]) and torch.equal(count, b.count)


def test_pad_rows():
    assert pad_rows([[1, 2, 3], [], [4]], -1).tolist() == [[1, 2, 3], [-1, -1, -1], [4, -1, -1]]
    assert pad_rows([[], []], -1).tolist() == [[-1], [-1]] and pad_rows([[], []], -1).dtype == np.int32
    wide = pad_rows([[1], [2, 3]], 0, np.int64, (3, 4))
    assert wide.dtype == np.int64 and wide.tolist() == [[1, 0, 0, 0], [2, 3, 0, 0], [0, 0, 0, 0]]


def test_check_leads():
    for ok in (1, 12, np.int64(3)):
        check_leads(ok, "beat detection")
    check_leads(65535, "beat classes", 65535)
    for bad in (0, -1, True, 2.0, "2", None):
        with pytest.raises(RalError, match=r"^beat detection: leads must be >= 1 \(got "):
            check_leads(bad, "beat detection")
    with pytest.raises(RalError, match=r"^beat classes: leads must be in \[1, 65535\] \(got 65536\)$"):
        check_leads(65536, "beat classes", 65535)
