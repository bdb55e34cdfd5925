"""What the tests of the fused U-Net inference kernel (k_unet_infer) share, all of it on the CPU: a BatchNorm state that is
away from the 0 / 1 defaults, a batch that gives every workgroup of the persistent grid at least two windows whatever the
occupancy query answers, the windows compared bit for bit, the fp64 reference and the per-window error.

The reference evaluates the oracle with the numbers the handle holds: the fp32 parameters and the fp32 roundings of the warmed
running statistics, both cast to fp64."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

import ralenet_oracle as O

CU_LDS = 163840            # LDS bytes of a compute unit
CU_WORKGROUPS = 8          # 32 wave slots of a compute unit over workgroups of four waves
FUSED_L = (256, 512, 768, 1024)
CASES = [(leads, L) for leads in (1, 2) for L in FUSED_L]
SEED, DATA_SEED, PASSES, WINDOWS = 1234, 7, 30, 64

_STATE, _INPUT, _REF = {}, {}, {}


def warmed_state(leads, L, seed=SEED, data_seed=DATA_SEED, passes=PASSES, windows=WINDOWS):
    """(p32, bn): the fp32 parameters of O.init_params(O.unet_param_shapes(leads), seed) and the state of O.unet_bn_state (fp64)
    after `passes` fp64 training forwards of O.unet_forward over `windows` standard-normal windows (the same windows every pass:
    after 30 passes the running statistics are 96 % those of the data, 4 % the defaults)"""
    key = (leads, L, seed, data_seed, passes, windows)
    if key not in _STATE:
        p32 = O.init_params(O.unet_param_shapes(leads), seed)
        p64 = OrderedDict((k, v.double()) for k, v in p32.items())
        bn = O.unet_bn_state(p64, torch.float64)
        g = torch.Generator().manual_seed(data_seed)
        xw = torch.randn(windows, leads, L, generator=g).double()
        with torch.no_grad():
            for _ in range(passes):
                O.unet_forward(p64, xw, True, bn)
        _STATE[key] = (p32, bn)
    return _STATE[key]


def flat_state_dict(p32, bn):
    """the warmed state as UNet.load_state_dict(..., strict=False) takes it: parameters, <bn>.running_mean, <bn>.running_var"""
    sd = OrderedDict(p32)
    for k in O.UNET_BN:
        for s in ("running_mean", "running_var"):
            sd[k + "." + s] = bn[k][s]
    return sd


def warmed_state_dict(leads, L, **kw):
    return flat_state_dict(*warmed_state(leads, L, **kw))


def case_input(leads, L, B, data_seed=DATA_SEED, windows=WINDOWS):
    """B standard-normal windows (fp32, CPU) from the generator of the warm-up, drawn after the warm-up windows"""
    key = (leads, L, B, data_seed, windows)
    if key not in _INPUT:
        g = torch.Generator().manual_seed(data_seed)
        torch.randn(windows, leads, L, generator=g)
        _INPUT[key] = torch.randn(B, leads, L, generator=g)
    return _INPUT[key]


def oracle_eval(leads, L, x, dtype=torch.float64, **kw):
    """the oracle's eval forward of the windows x from the warmed state as a handle holds it (fp32 roundings), in `dtype`"""
    p32, bn = warmed_state(leads, L, **kw)
    p = OrderedDict((k, v.to(dtype)) for k, v in p32.items())
    held = {k: {s: bn[k][s].float().to(dtype) for s in ("running_mean", "running_var")} for k in O.UNET_BN}
    with torch.no_grad():
        return O.unet_forward(p, x.to(dtype), False, held)


def case_reference(leads, L, B):
    """(x, fp64 eval output) of the case's B windows, computed once"""
    key = (leads, L, B)
    if key not in _REF:
        x = case_input(leads, L, B)
        _REF[key] = (x, oracle_eval(leads, L, x))
    return _REF[key]


def window_errors(y, ref):
    """e[w] = |y[w] - ref[w]| / |ref[w]| over the window's leads * L samples, in fp64"""
    y, ref = torch.as_tensor(y).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return ((y - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)).numpy()


def fused_plan(leads, L, B, fused=1):
    """(kernel name, threads, LDS bytes, fused_eval) of the eval forward as one kernel, from ral_unet_stage_plan (stage -1)"""
    from ecg_denoise_amd import _lib
    lib = _lib.lib()
    name = C.create_string_buffer(64)
    grid, th, wp, fold, fe = (C.c_int32() for _ in range(5))
    lds = C.c_int64()
    rc = lib.ral_unet_stage_plan(0, leads, L, B, 0, -1, fused, name, len(name), C.byref(grid), C.byref(th), C.byref(wp), C.byref(lds),
                                 C.byref(fold), C.byref(fe))
    assert rc == 0, lib.ral_last_error()
    return name.value.decode(), th.value, lds.value, fe.value


def resident_bound(leads, L, cus):
    """the most workgroups of k_unet_infer<leads> that can be resident at once, from what a test knows without asking the kernel:
    a CU's LDS over the plan's LDS bytes, and its 32 wave slots over four-wave workgroups.  Registers and allocation granules can
    only lower the true figure."""
    name, threads, lds, fe = fused_plan(leads, L, 1)
    assert fe == 1 and name == "k_unet_infer<%d>" % leads and threads == 256 and 0 < lds <= CU_LDS, (name, threads, lds, fe)
    return cus * min(CU_LDS // lds, CU_WORKGROUPS)


def wrap_batch(leads, L, cus):
    """more than twice the bound: every workgroup takes a second window; the ragged 37: some take a third and some do not"""
    return 2 * resident_bound(leads, L, cus) + 37


def pass_windows(B, cus):
    """the windows compared bit for bit: around every multiple of the CU count (whatever workgroups per CU the occupancy query
    answers, a workgroup's second, third ... window starts at one of them) and around the ragged tail"""
    idx = {0, 1, cus - 1, cus, cus + 1, 2 * cus - 1, 2 * cus, B - 38, B - 37, B - 1}
    for m in range(3 * cus, B, cus):
        idx |= {m - 1, m, m + 1}
    return sorted(i for i in idx if 0 <= i < B)


def signal_share(y):
    """per window |y - mean_t(y)| / |y|: how much of the output is signal, not a per-lead constant"""
    y = y.double()
    return ((y - y.mean(-1, keepdim=True)).flatten(1).norm(dim=1) / y.flatten(1).norm(dim=1)).numpy()


def stats_range(bn):
    means = np.concatenate([bn[k]["running_mean"].numpy() for k in O.UNET_BN])
    var = np.concatenate([bn[k]["running_var"].numpy() for k in O.UNET_BN])
    return means.min(), means.max(), var.min(), var.max()
