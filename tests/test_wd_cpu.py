"""CPU: weight decay on the device -- the nef_update C-ABI entry, the decay run table and the Python surface (no GPU work)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Cfg(dict):
    __getattr__ = dict.__getitem__


def test_header_declares_nef_update_and_binding_has_it():
    from electrocardio_panorama_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    assert re.search(r"\bint nef_update\s*\(\s*const nef_update_args\s*\*", hdr)
    assert re.search(r"typedef struct nef_update_args\s*\{", hdr) and re.search(r"\}\s*nef_update_args\s*;", hdr)
    assert re.search(r"#define NEF_UPDATE_MAX_RUNS 256\b", hdr)
    assert "CALLER'S DUTY" in hdr          # the entry cannot read device memory: the table's consistency is not checked
    L = _lib.load()
    for name in ("nef_update", "nef_update_args_bytes"):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
    assert ctypes.sizeof(_lib.UpdateArgs) == 144 == L.nef_update_args_bytes()
    assert L.nef_abi_version() == 22       # the change was additive (ABI 21 then; 22 since the single-operand packing entries went)


def _args(**kw):
    from electrocardio_panorama_amd import _lib
    a = _lib.UpdateArgs(p=64, g=64, buf=64, m=64, v=64, step=64, n=16, lr=0.1, gscale=1.0, mu=0.9, beta1=0.9, beta2=0.999, eps=1e-8)
    for k, v in kw.items():
        setattr(a, k, v)
    return ctypes.byref(a)


def test_nef_update_rejects_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the first launch, so the (non-NULL, never dereferenced) addresses are not read."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    assert L.nef_update(None, None) == -2                                     # NEF_E_NULL
    assert L.nef_update(_args(p=None), None) == -2
    assert L.nef_update(_args(g=None), None) == -2
    assert L.nef_update(_args(rule=0, buf=None), None) == -2
    for rule in (1, 2):
        for k in ("m", "v", "step"):
            assert L.nef_update(_args(rule=rule, **{k: None}), None) == -2
    assert L.nef_update(_args(rule=3), None) == -4                            # NEF_E_UNSUPPORTED
    for rule in (0, 1, 2):
        assert L.nef_update(_args(rule=rule, n_runs=257, run_end=64, run_mul=64), None) == -1     # NEF_E_SHAPE: above the cap
        assert L.nef_update(_args(rule=rule, n_runs=-1), None) == -1
        assert L.nef_update(_args(rule=rule, n=0), None) == -1
        assert L.nef_update(_args(rule=rule, weight_decay=-0.1), None) == -1
        assert L.nef_update(_args(rule=rule, n_runs=2, run_end=64), None) == -2                   # a table is both arrays


def test_default_config_has_decay_off():
    from electrocardio_panorama_amd.config import get_defaults
    s = get_defaults().SOLVER
    assert s.weight_decay == 0.0 and s.nesterov is False and s.no_decay == []
    cfg = get_defaults()
    cfg.merge_from_list(["SOLVER.optim", "adamw", "SOLVER.weight_decay", "1e-2", "SOLVER.nesterov", True, "SOLVER.no_decay", "['*.bias']"])
    assert cfg.SOLVER.optim == "adamw" and cfg.SOLVER.weight_decay == 0.01 and cfg.SOLVER.nesterov is True
    assert cfg.SOLVER.no_decay == ["*.bias"]


def test_get_optimizer_maps_the_keys():
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam, FusedAdamW, FusedSGD, get_optimizer
    params = [torch.nn.Parameter(torch.zeros(3))]
    # configs written before the keys existed
    for name, cls in (("sgd", FusedSGD), ("adam", FusedAdam), ("adamw", FusedAdamW)):
        opt = get_optimizer(Cfg(SOLVER=Cfg(optim=name, lr=1e-3)), params)
        assert type(opt) is cls and opt.no_decay == () and opt.param_groups[0]["weight_decay"] == 0
    assert get_optimizer(Cfg(SOLVER=Cfg(optim="sgd", lr=1e-3)), params).param_groups[0]["nesterov"] is False
    # ... and with them
    s = Cfg(optim="sgd", lr=0.1, weight_decay=0.05, nesterov=True, no_decay=["*.bias", "bn.*"], clip_grad_norm=0.5)
    opt = get_optimizer(Cfg(SOLVER=s), params)
    g = opt.param_groups[0]
    assert type(opt) is FusedSGD and g["weight_decay"] == 0.05 and g["nesterov"] is True and g["momentum"] == 0.9 and g["dampening"] == 0
    assert opt.no_decay == ("*.bias", "bn.*") and opt.max_grad_norm == 0.5
    # an optimiser attribute, not a parameter-group key: the state dict stays in torch's format
    assert "no_decay" not in g and "no_decay" not in opt.state_dict()["param_groups"][0]
    assert set(g) == set(torch.optim.SGD(params, lr=0.1).param_groups[0])
    s["optim"] = "adam"
    opt = get_optimizer(Cfg(SOLVER=s), params)
    g = opt.param_groups[0]
    assert type(opt) is FusedAdam and g["weight_decay"] == 0.05 and not g.get("decoupled_weight_decay") and opt.no_decay == ("*.bias", "bn.*")
    s["optim"] = "adamw"
    opt = get_optimizer(Cfg(SOLVER=s), params)
    g = opt.param_groups[0]
    assert type(opt) is FusedAdamW and g["weight_decay"] == 0.05 and g["decoupled_weight_decay"] is True
    assert set(g) == set(torch.optim.AdamW(params).param_groups[0])
    assert FusedAdamW(params).param_groups[0]["weight_decay"] == 1e-2          # torch.optim.AdamW's default


def test_validation_errors():
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam, FusedAdamW, FusedSGD
    params = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        FusedSGD(params, lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError):
        FusedSGD(params, lr=0.1, dampening=0.1, nesterov=True)
    with pytest.raises(ValueError):
        FusedSGD(params, lr=0.1, weight_decay=-1e-3)
    with pytest.raises(NotImplementedError):
        FusedSGD(params, lr=0.1, dampening=0.1)
    with pytest.raises(ValueError):
        FusedAdamW(params, weight_decay=-1e-3)
    for cls in (FusedAdam, FusedAdamW):
        with pytest.raises(NotImplementedError):
            cls(params, amsgrad=True)
        with pytest.raises(NotImplementedError):
            cls(params, maximize=True)
    # checkpoints of what is not implemented are refused, not stepped as something else
    with pytest.raises(NotImplementedError):
        FusedAdam(params).load_state_dict(torch.optim.AdamW(params).state_dict())          # a decoupled group
    with pytest.raises(NotImplementedError):
        FusedAdamW(params).load_state_dict(torch.optim.AdamW(params, amsgrad=True).state_dict())
    with pytest.raises(NotImplementedError):
        FusedSGD(params, lr=0.1).load_state_dict(torch.optim.SGD(params, lr=0.1, momentum=0.9, dampening=0.5).state_dict())
    # ... and torch's own checkpoints of what is implemented load
    FusedAdamW(params).load_state_dict(torch.optim.AdamW(params).state_dict())
    FusedSGD(params, lr=0.1).load_state_dict(torch.optim.SGD(params, lr=0.1, momentum=0.9, weight_decay=0.1, nesterov=True).state_dict())


def test_decay_runs():
    from electrocardio_panorama_amd.solver.optim_scheduler import decay_runs
    names = ["a.weight", "a.bias", "b.weight", "b.bias", "decoder.4.bias"]
    sizes = [12, 3, 20, 5, 1]
    assert decay_runs(names, sizes, ()) == ([], [])                              # no pattern: no table
    assert decay_runs(names, sizes, ["nothing.*"]) == ([], [])                   # nothing exempt: no table
    assert decay_runs(names, sizes, ["*.bias"]) == ([12, 15, 35, 41], [1.0, 0.0, 1.0, 0.0])      # b.bias + the size-1 tensor merge
    assert decay_runs(names, sizes, ["decoder.4.bias"]) == ([40, 41], [1.0, 0.0])                # neighbours merge; a one-element run
    assert decay_runs(names, sizes, ["a.*", "b.weight"]) == ([35, 41], [0.0, 1.0])
    assert decay_runs(names, sizes, ["*"]) == ([41], [0.0])                      # all exempt
    assert decay_runs([None, "x.bias"], [4, 2], ["*"]) == ([4, 6], [1.0, 0.0])   # an unnamed tensor is never exempt
    assert decay_runs(["w", "e.bias", "z.bias"], [4, 0, 2], ["*.bias"]) == ([4, 6], [1.0, 0.0])   # an empty tensor makes no run
    # fnmatch is case-sensitive here, whatever the platform
    assert decay_runs(["A.Bias"], [3], ["*.bias"]) == ([], [])


def test_decay_runs_on_the_model_exempt_exactly_the_1d_parameters():
    from electrocardio_panorama_amd.config import get_defaults
    from electrocardio_panorama_amd.network import build_model
    from electrocardio_panorama_amd.solver.optim_scheduler import MAX_RUNS, decay_runs
    cfg = get_defaults()
    cfg.MODEL.model = "model_nefnet"
    cfg.DATA.lead_num = 3
    m = build_model(cfg)
    named = list(m.named_parameters())
    assert len(named) == 53 and all(p._nef_name == k for k, p in named)
    names, sizes = [k for k, _ in named], [p.numel() for _, p in named]
    assert sizes[names.index("decoder.4.bias")] == 1
    ends, muls = decay_runs(names, sizes, ["*.bias", "decoder.*.double_conv.[14].weight"])
    assert ends[-1] == sum(sizes) and ends == sorted(set(ends)) and 1 < len(ends) <= MAX_RUNS
    assert all(a != b for a, b in zip(muls, muls[1:]))                           # merged
    off = 0
    for (k, p), n in zip(named, sizes):
        r = next(i for i, e in enumerate(ends) if e > off)
        assert ends[r] >= off + n, k                                             # a tensor lies in one run
        assert muls[r] == (0.0 if p.dim() == 1 else 1.0), (k, tuple(p.shape))
        off += n
