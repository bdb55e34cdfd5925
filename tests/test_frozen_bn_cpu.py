"""Host side of fine-tuning with frozen BatchNorm statistics, as far as it runs without a device: `train(freeze_bn=...)`,
`NewRALE(freeze_bn=...)`, what the networks without the option answer, and the shape of the C ABI - the feature is a key of
`ral_set_option`, it adds no export and changes no signature."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from ecg_denoise_amd import _lib
from ecg_denoise_amd import model as M
from ecg_denoise_amd.train import train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the 90 functions of the C ABI before this option existed
EXPORTS_BEFORE = """ral_adam_flat ral_adam_step ral_arrhythmia_windows ral_attention_backward ral_attention_backward_scratch_floats
ral_attention_forward ral_attention_plan ral_backward ral_backward_begin ral_backward_end ral_backward_input ral_backward_input_begin
ral_backward_input_end ral_baseline_layer_geom ral_baseline_pass_plan ral_beat_match ral_beat_pool ral_beat_records
ral_beat_records_scratch_bytes ral_bind ral_block_plan ral_bn_sums_doubles ral_conv13_backward ral_conv13_forward ral_create
ral_debug_tensor ral_delineate_records ral_destroy ral_fft_denoise ral_fft_denoise_scratch_bytes ral_forward ral_forward_begin
ral_forward_end ral_forward_loss_means ral_global_option ral_grad_bucket ral_grad_bucket_wait ral_hrv_windows ral_last_error
ral_layout_count ral_layout_entry ral_live_emit ral_live_windows ral_loss ral_loss_flat ral_loss_mean ral_loss_means ral_mix_batch
ral_mix_draw ral_mix_records ral_mix_records_scratch_bytes ral_newrale_live_back ral_newrale_live_front ral_newrale_pool_back
ral_newrale_pool_front ral_newrale_stream_back ral_newrale_stream_front ral_param_floats ral_pe_table ral_pool_emit ral_pool_windows
ral_prep_windows ral_profile_read ral_profile_select ral_profile_timeline ral_pst_records ral_ralenet_node_geom
ral_ralenet_pass_plan ral_rate_pool ral_rate_records ral_rhythm_pool ral_rhythm_pool_scratch_bytes ral_rhythm_records
ral_score_records ral_score_records_scratch_bytes ral_set_option ral_state_floats ral_stream_stitch ral_stream_windows
ral_template_records ral_unet_backward_finish ral_unet_backward_stage ral_unet_backward_start ral_unet_forward_finish
ral_unet_forward_stage ral_unet_stage_bn ral_unet_stage_geom ral_unet_stage_plan ral_wavelet_denoise ral_workspace_bytes""".split()


class FakeModel:
    """what `train` touches, recording the order of the calls"""

    def __init__(self):
        self.calls = []
        self.device = torch.device("cpu")

    def freeze_bn(self, flag=True):
        self.calls.append(("freeze_bn", flag))
        return self

    def train(self, mode=True):
        self.calls.append(("train", mode))
        return self

    def eval(self):
        return self.train(False)

    def train_step(self, x, t, lr):
        self.calls.append(("train_step",))
        z = torch.zeros(1)
        return {"loss": z.double(), "snr": z, "rmse": z}

    def __call__(self, x):
        return x

    def loss_and_metrics(self, pred, target, want_grad=True):
        z = torch.zeros(1)
        return z.double(), z, z

    def state_dict(self):
        return {}


def _run_train(tmp_path, monkeypatch, **kw):
    monkeypatch.chdir(tmp_path)                      # (train appends a line to output.txt under out_dir)
    m = FakeModel()
    batches = [(torch.zeros(1, 2, 16), torch.zeros(1, 2, 16))] * 2
    train(1, m, 1, batches, batches, model_name="fake", noise_name="n", noise_intensity=0, out_dir=str(tmp_path),
          log=lambda *a, **k: None, **kw)
    return m.calls


@pytest.mark.parametrize("flag", [True, False])
def test_train_freezes_before_the_first_step(tmp_path, monkeypatch, flag):
    calls = _run_train(tmp_path, monkeypatch, freeze_bn=flag)
    assert calls.count(("freeze_bn", flag)) == 1 and len([c for c in calls if c[0] == "freeze_bn"]) == 1
    assert calls.index(("freeze_bn", flag)) < calls.index(("train_step",))
    assert calls.count(("train_step",)) == 2


def test_train_without_the_argument_makes_no_call(tmp_path, monkeypatch):
    for kw in ({}, {"freeze_bn": None}):
        calls = _run_train(tmp_path, monkeypatch, **kw)
        assert not [c for c in calls if c[0] == "freeze_bn"] and calls.count(("train_step",)) == 2


def _fake_inner(leads=2):
    inner = types.SimpleNamespace(eng=types.SimpleNamespace(leads=leads, device=torch.device("cpu"), L=32), calls=[], frozen=False)

    def freeze_bn(flag=True):
        inner.calls.append(flag)
        inner.frozen = bool(flag)
        return inner
    inner.freeze_bn = freeze_bn
    return inner


def test_newrale_argument_reaches_the_inner_model():
    a = _fake_inner()
    M.NewRALE(a, seed=1)
    assert a.calls == [], "freeze_bn=False is the reference's behaviour (quirk A16): the inner model is left as it is"
    b = _fake_inner()
    m = M.NewRALE(b, seed=1, freeze_bn=True)
    assert b.calls == [True]
    assert m.freeze_bn(False) is m and b.calls == [True, False]
    doc = M.NewRALE.__doc__
    assert "freeze_bn=True" in doc and "A16" in doc and "matches inference" in doc


def test_networks_without_frozen_statistics():
    d = object.__new__(M.DANet)                      # (no handle: the refusal comes before anything is touched)
    with pytest.raises(_lib.RalError, match="not provided"):
        d.freeze_bn(True)
    with pytest.raises(_lib.RalError, match="not provided"):
        d.freeze_bn()
    assert d.freeze_bn(False) is d and d.bn_frozen is False
    a = object.__new__(M.ACDAE)                      # no BatchNorm: a no-op either way
    assert a.freeze_bn() is a and a.freeze_bn(False) is a and a.bn_frozen is False
    for cls in (M.RALENet, M.UNet):
        assert cls.freeze_bn is M._ModuleBase.freeze_bn and isinstance(cls.bn_frozen, property)


def test_the_c_abi_lists_the_functions_it_listed_before():
    assert sorted(_lib.EXPORTS) == sorted(EXPORTS_BEFORE) and len(EXPORTS_BEFORE) == 90
    assert sorted(_lib._SIGS) == sorted(EXPORTS_BEFORE)
    hdr = open(os.path.join(ROOT, "include", "ralenet.h")).read()
    declared = set(re.findall(r"\b(ral_[a-z_0-9]+)\s*\(", hdr)) - {"ral_handle"}
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    restype, argtypes = _lib._SIGS["ral_set_option"]
    assert restype is C.c_int and list(argtypes) == [C.c_void_p, C.c_char_p, C.c_int]


def test_the_option_is_documented_with_ral_set_option():
    hdr = open(os.path.join(ROOT, "include", "ralenet.h")).read()
    end = hdr.index("int ral_set_option(")
    comment = hdr[hdr.rindex("/*", 0, end):end]
    assert '"bn_frozen"' in comment
    for word in ("running_mean", "running_var", "bn_sums", "changed since the", "U-Net", "DANet"):
        assert word in comment, word
