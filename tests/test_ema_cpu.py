"""CPU: the EMA of the weights on the device -- the nef_update_ema C-ABI entry, its argument checks and the Python surface (no GPU work)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Cfg(dict):
    __getattr__ = dict.__getitem__


def test_header_declares_nef_update_ema_and_binding_has_it():
    from electrocardio_panorama_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    assert re.search(r"typedef struct nef_ema_args\s*\{", hdr) and re.search(r"\}\s*nef_ema_args\s*;", hdr)
    assert re.search(r"\bint nef_update_ema\s*\(\s*const nef_update_args\s*\*\s*\w+\s*,\s*const nef_ema_args\s*\*", hdr)
    assert re.search(r"\bsize_t nef_ema_args_bytes\s*\(\s*void\s*\)", hdr)
    L = _lib.load()
    for name in ("nef_update_ema", "nef_ema_args_bytes"):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
    assert ctypes.sizeof(_lib.EmaArgs) == L.nef_ema_args_bytes()
    # the change was additive (ABI 21 then; 22 since the single-operand packing entries went)
    assert L.nef_abi_version() == 22
    assert ctypes.sizeof(_lib.UpdateArgs) == 144 == L.nef_update_args_bytes()


def _args(**kw):
    from electrocardio_panorama_amd import _lib
    a = _lib.UpdateArgs(p=64, g=64, buf=64, m=64, v=64, step=64, n=16, lr=0.1, gscale=1.0, mu=0.9, beta1=0.9, beta2=0.999, eps=1e-8)
    for k, v in kw.items():
        setattr(a, k, v)
    return ctypes.byref(a)


def _ema(**kw):
    from electrocardio_panorama_amd import _lib
    e = _lib.EmaArgs(ema=64, n_averaged=64, decay=0.999, warmup=0)
    for k, v in kw.items():
        setattr(e, k, v)
    return ctypes.byref(e)


def test_nef_update_ema_rejects_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the first launch, so the (non-NULL, never dereferenced) addresses are not read."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    for rule in (0, 1, 2):
        assert L.nef_update_ema(_args(rule=rule), None, None) == -2                               # NEF_E_NULL
        assert L.nef_update_ema(_args(rule=rule), _ema(ema=None), None) == -2
        assert L.nef_update_ema(_args(rule=rule), _ema(n_averaged=None), None) == -2
        for decay in (1.0, 1.5, -0.1, float("nan"), float("inf")):
            assert L.nef_update_ema(_args(rule=rule), _ema(decay=decay), None) == -1              # NEF_E_SHAPE
    # ... and everything nef_update rejects, the same way
    assert L.nef_update_ema(None, _ema(), None) == -2
    assert L.nef_update_ema(_args(p=None), _ema(), None) == -2
    assert L.nef_update_ema(_args(g=None), _ema(), None) == -2
    assert L.nef_update_ema(_args(rule=0, buf=None), _ema(), None) == -2
    for rule in (1, 2):
        for k in ("m", "v", "step"):
            assert L.nef_update_ema(_args(rule=rule, **{k: None}), _ema(), None) == -2
    assert L.nef_update_ema(_args(rule=3), _ema(), None) == -4                                    # NEF_E_UNSUPPORTED
    for rule in (0, 1, 2):
        assert L.nef_update_ema(_args(rule=rule, n_runs=257, run_end=64, run_mul=64), _ema(), None) == -1
        assert L.nef_update_ema(_args(rule=rule, n_runs=-1), _ema(), None) == -1
        assert L.nef_update_ema(_args(rule=rule, n=0), _ema(), None) == -1
        assert L.nef_update_ema(_args(rule=rule, weight_decay=-0.1), _ema(), None) == -1
        assert L.nef_update_ema(_args(rule=rule, n_runs=2, run_end=64), _ema(), None) == -2


def test_default_config_has_ema_off():
    from electrocardio_panorama_amd.config import get_defaults
    s = get_defaults().SOLVER
    assert s.ema_decay == 0.0 and s.ema_warmup is False and s.ema_eval is True
    cfg = get_defaults()
    cfg.merge_from_list(["SOLVER.ema_decay", "0.999", "SOLVER.ema_warmup", True, "SOLVER.ema_eval", False])
    assert cfg.SOLVER.ema_decay == 0.999 and cfg.SOLVER.ema_warmup is True and cfg.SOLVER.ema_eval is False


def test_get_optimizer_maps_the_keys():
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam, FusedAdamW, FusedSGD, get_optimizer
    params = [torch.nn.Parameter(torch.zeros(3))]
    for name, cls in (("sgd", FusedSGD), ("adam", FusedAdam), ("adamw", FusedAdamW)):
        opt = get_optimizer(Cfg(SOLVER=Cfg(optim=name, lr=1e-3)), params)          # a config written before the keys existed
        assert type(opt) is cls and opt.ema_decay == 0.0 and opt.ema_warmup is False
        opt = get_optimizer(Cfg(SOLVER=Cfg(optim=name, lr=1e-3, ema_decay=0.99, ema_warmup=True)), params)
        assert type(opt) is cls and opt.ema_decay == 0.99 and opt.ema_warmup is True
        # a change of either re-captures a graphed step
        g = opt.param_groups[0]
        before = opt._captured_scalars(g)
        opt.ema_decay = 0.9
        assert opt._captured_scalars(g) != before


@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_ema_decay_outside_0_1_raises(kind):
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam, FusedAdamW, FusedSGD
    cls = {"sgd": FusedSGD, "adam": FusedAdam, "adamw": FusedAdamW}[kind]
    params = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            cls(params, lr=0.1, ema_decay=bad)
    cls(params, lr=0.1, ema_decay=0.0)
    cls(params, lr=0.1, ema_decay=0.9999, ema_warmup=True)


@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_state_dict_keeps_torchs_format_with_ema_on(kind):
    """ema_decay / ema_warmup are attributes of the optimiser, not parameter-group keys."""
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam, FusedAdamW, FusedSGD
    cls = {"sgd": FusedSGD, "adam": FusedAdam, "adamw": FusedAdamW}[kind]
    params = [torch.nn.Parameter(torch.zeros(3))]
    off, on = cls(params, lr=0.1).state_dict(), cls(params, lr=0.1, ema_decay=0.999, ema_warmup=True).state_dict()
    assert set(off) == set(on) == {"state", "param_groups"}
    assert [set(g) for g in off["param_groups"]] == [set(g) for g in on["param_groups"]]
    assert not any(k.startswith("ema") for g in on["param_groups"] for k in g)
    ref = {"sgd": torch.optim.SGD(params, lr=0.1), "adam": torch.optim.Adam(params), "adamw": torch.optim.AdamW(params)}[kind]
    assert set(on["param_groups"][0]) <= set(ref.state_dict()["param_groups"][0]) | {"decoupled_weight_decay"}


def test_ema_surface_before_the_first_step():
    """ema_weights() does nothing before the first step and with the average off; ema_state_dict() then holds the live tensors under
    exactly the model's keys; load_ema_state_dict keeps the tensors until the flat buffers are built."""
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedSGD
    model = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    for k, p in model.named_parameters():
        p._nef_name = k
    w0 = model[0].weight.detach().clone()
    for decay in (0.0, 0.9):
        opt = FusedSGD(model.parameters(), lr=0.1, ema_decay=decay)
        with opt.ema_weights():
            assert torch.equal(model[0].weight, w0)
        sd = opt.ema_state_dict(model)
        assert set(sd) == {"decay", "warmup", "n_averaged", "model"} and sd["decay"] == decay and sd["n_averaged"] == 0.0
        assert list(sd["model"]) == list(model.state_dict())
        assert all(torch.equal(sd["model"][k], v) for k, v in model.state_dict().items())
        sd["model"]["0.weight"] = w0 + 1.0
        sd["n_averaged"] = 7.0
        opt.load_ema_state_dict(sd)
        back = opt.ema_state_dict(model)
        if decay:
            assert back["n_averaged"] == 7.0 and torch.equal(back["model"]["0.weight"], w0 + 1.0)
        else:          # the average is off: nothing is kept
            assert back["n_averaged"] == 0.0 and torch.equal(back["model"]["0.weight"], w0)
