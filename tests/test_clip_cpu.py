"""CPU: the C-ABI entry of the global gradient-norm clipping and its Python surface (no GPU work)."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Cfg(dict):
    __getattr__ = dict.__getitem__


def test_header_declares_nef_grad_clip_and_binding_has_it():
    from electrocardio_panorama_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    assert re.search(r"\bint nef_grad_clip\s*\(", hdr)
    assert re.search(r"\bsize_t nef_grad_clip_ws_bytes\s*\(", hdr)
    for name in ("nef_grad_clip", "nef_grad_clip_ws_bytes"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)


def test_nef_grad_clip_rejects_bad_arguments_without_touching_the_gpu():
    """NULL g / stats / ws -> NEF_E_NULL; max_norm <= 0 or NaN -> NEF_E_SHAPE: every check sits in front of the first launch, so the
    (non-NULL, never dereferenced) addresses below are not read."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    n = L.nef_grad_clip_ws_bytes()
    assert n > 0
    assert L.nef_grad_clip(None, 16, 1.0, 1.0, None, None, None, n, None) == -2
    assert L.nef_grad_clip(None, 16, 1.0, 1.0, None, 64, 64, n, None) == -2       # g
    assert L.nef_grad_clip(64, 16, 1.0, 1.0, None, None, 64, n, None) == -2       # stats
    assert L.nef_grad_clip(64, 16, 1.0, 1.0, None, 64, None, n, None) == -2       # ws
    for bad in (0.0, -1.0, math.nan):
        assert L.nef_grad_clip(64, 16, bad, 1.0, None, 64, 64, n, None) == -1
    assert L.nef_grad_clip(64, 0, 1.0, 1.0, None, 64, 64, n, None) == -1
    assert L.nef_grad_clip(64, 16, 1.0, 1.0, None, 64, 64, n - 1, None) == -3     # NEF_E_WORKSPACE


def test_default_config_has_clipping_off():
    from electrocardio_panorama_amd.config import get_defaults
    assert get_defaults().SOLVER.clip_grad_norm == 0.0


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_get_optimizer_carries_clip_grad_norm(name):
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    params = [torch.nn.Parameter(torch.zeros(3))]
    opt = get_optimizer(Cfg(SOLVER=Cfg(optim=name, lr=1e-3)), params)          # a config written before the key existed
    assert opt.max_grad_norm == 0 and opt.clip_stats is None
    opt = get_optimizer(Cfg(SOLVER=Cfg(optim=name, lr=1e-3, clip_grad_norm=0.25)), params)
    assert opt.max_grad_norm == 0.25
    # an optimiser attribute, not a parameter-group key: the state dict stays in torch's format
    assert "max_grad_norm" not in opt.state_dict()["param_groups"][0]
    assert "max_grad_norm" not in opt.param_groups[0]


def test_fused_optimisers_refuse_an_invalid_max_grad_norm():
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam, FusedSGD
    params = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (-1.0, math.nan):
        with pytest.raises(ValueError):
            FusedSGD(params, lr=0.1, max_grad_norm=bad)
        with pytest.raises(ValueError):
            FusedAdam(params, max_grad_norm=bad)
    assert FusedSGD(params, lr=0.1, max_grad_norm=math.inf).max_grad_norm == math.inf
