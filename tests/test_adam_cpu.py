"""CPU: the fused Adam optimiser's C-ABI entry and its Python surface (no GPU work)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Cfg(dict):
    __getattr__ = dict.__getitem__


def test_header_declares_nef_adam_and_binding_has_it():
    from electrocardio_panorama_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    assert re.search(r"\bint nef_adam\s*\(", hdr)
    assert "nef_adam" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "nef_adam")


def test_nef_adam_rejects_null_without_touching_the_gpu():
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    assert L.nef_adam(None, None, None, None, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None, None, None, None, None) == -2  # NEF_E_NULL


def test_get_optimizer_adam_returns_fused_adam():
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam, FusedSGD, get_optimizer
    params = [torch.nn.Parameter(torch.zeros(3))]
    cfg = Cfg(SOLVER=Cfg(optim="adam", lr=1e-3))
    opt = get_optimizer(cfg, params)
    assert isinstance(opt, FusedAdam)
    g = opt.param_groups[0]
    assert g["lr"] == 1e-3 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and g["weight_decay"] == 0
    assert g["amsgrad"] is False and g["maximize"] is False
    cfg.SOLVER["optim"] = "sgd"
    assert isinstance(get_optimizer(cfg, params), FusedSGD)


def test_fused_adam_refuses_what_it_does_not_implement():
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam
    params = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError):
        FusedAdam(params, amsgrad=True)
    with pytest.raises(NotImplementedError):
        FusedAdam(params, maximize=True)
    with pytest.raises(ValueError):
        FusedAdam(params, betas=(1.0, 0.999))
    # a torch checkpoint that asks for AMSGrad is refused rather than silently stepped without it
    ref = torch.optim.Adam(params, lr=1e-3, amsgrad=True)
    opt = FusedAdam(params)
    with pytest.raises(NotImplementedError):
        opt.load_state_dict(ref.state_dict())
