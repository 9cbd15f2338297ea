"""CPU: gradient accumulation (SOLVER.accum_steps) -- the nef_flatten_acc C-ABI entry, its argument checks and the Python surface
(no GPU work)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Cfg(dict):
    __getattr__ = dict.__getitem__


def test_header_declares_the_entry_and_binding_has_it():
    from electrocardio_panorama_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    assert re.search(r"\bint nef_flatten_acc\s*\(\s*const float\s*\*\s*const\s*\*\s*srcs,\s*const int64_t\s*\*\s*sizes,\s*int n,\s*float\s*\*\s*out,"
                     r"\s*int accumulate,\s*const int32_t\s*\*\s*accumulate_dev,\s*nef_stream_t stream\s*\)", hdr)
    # nef_flatten is declared as it was
    assert "int nef_flatten(const float* const* srcs, const int64_t* sizes, int n, float* out, nef_stream_t stream);" in hdr
    doc = hdr[:hdr.index("int nef_flatten_acc")].rsplit("/*", 1)[1]
    assert "HOST" in doc and "+=" in doc and "never read" in doc
    L = _lib.load()
    assert "nef_flatten_acc" in _lib.SIGNATURES and hasattr(L, "nef_flatten_acc")
    assert len(_lib.SIGNATURES["nef_flatten_acc"][1]) == 7
    assert _lib.SIGNATURES["nef_flatten"] == (_lib.i32, [ctypes.POINTER(_lib.p), ctypes.POINTER(_lib.i64), _lib.i32, _lib.p, _lib.p])
    assert L.nef_abi_version() == 22          # additive


def _call(n, srcs="ok", sizes="ok", out=64, accumulate=0, vals=None, ptrs=None):
    """nef_flatten_acc with a NULL stream and (non-NULL, never dereferenced) device addresses."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    k = max(n, 1) if vals is None else len(vals)
    s = (ctypes.c_void_p * k)(*(ptrs if ptrs is not None else [64] * k)) if srcs == "ok" else None
    z = (ctypes.c_int64 * k)(*(vals if vals is not None else [4] * k)) if sizes == "ok" else None
    return L.nef_flatten_acc(s, z, n, out, accumulate, None, None)


def test_nef_flatten_acc_rejects_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the first launch, so nothing is launched and no address is read."""
    assert _call(2, srcs=None) == -2                       # NEF_E_NULL
    assert _call(2, sizes=None) == -2
    assert _call(2, out=None) == -2
    assert _call(-1) == -1                                 # NEF_E_SHAPE
    assert _call(-1, srcs=None, sizes=None, out=None) == -1
    assert _call(2, vals=[4, -1]) == -1
    assert _call(2, accumulate=2) == -1 and _call(2, accumulate=-1) == -1
    # ... also behind the 64th tensor, in front of what would be the first launch
    assert _call(70, vals=[4] * 69 + [-3]) == -1
    assert _call(70, vals=[4] * 70, ptrs=[64] * 69 + [None]) == -2
    # n == 0: nothing to do, whatever the pointers are
    assert _call(0) == 0 and _call(0, srcs=None, sizes=None, out=None) == 0
    assert _call(0, accumulate=1) == 0


def test_config_default_is_off():
    from electrocardio_panorama_amd.config import get_defaults
    assert get_defaults().SOLVER.accum_steps == 1
    cfg = get_defaults()
    cfg.merge_from_list(["SOLVER.accum_steps", "4"])
    assert cfg.SOLVER.accum_steps == 4


def _classes():
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam, FusedAdamW, FusedLAMB, FusedLARS, FusedSGD
    return {"sgd": (FusedSGD, dict(lr=0.1)), "adam": (FusedAdam, {}), "adamw": (FusedAdamW, {}), "lars": (FusedLARS, dict(lr=0.1)),
            "lamb": (FusedLAMB, {})}


@pytest.mark.parametrize("name", ["sgd", "adam", "adamw", "lars", "lamb"])
def test_constructors_validate_accum_steps(name):
    cls, kw = _classes()[name]
    params = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (0, -1, 1.5, True, "2", None, 2.0):
        with pytest.raises(ValueError):
            cls(params, accum_steps=bad, **kw)
    o = cls(params, **kw)
    assert o.accum_steps == 1 and not o.window_open
    o = cls(params, accum_steps=3, **kw)
    assert o.accum_steps == 3 and not o.window_open
    # an attribute like max_grad_norm: the state dict keeps torch's format
    assert "accum_steps" not in o.state_dict()["param_groups"][0] and "accum_steps" not in o.defaults
    o.flush()                                  # an empty window: nothing to do (and nothing built)
    assert o._flat == {}


@pytest.mark.parametrize("name", ["sgd", "adam", "adamw", "lars", "lamb"])
def test_get_optimizer_passes_the_key(name):
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    params = [torch.nn.Parameter(torch.zeros(3))]
    cls = _classes()[name][0]
    opt = get_optimizer(Cfg(SOLVER=Cfg(optim=name, lr=0.1)), params)              # a config written before the key existed
    assert type(opt) is cls and opt.accum_steps == 1
    opt = get_optimizer(Cfg(SOLVER=Cfg(optim=name, lr=0.1, accum_steps=4)), params)
    assert type(opt) is cls and opt.accum_steps == 4
    with pytest.raises(ValueError):
        get_optimizer(Cfg(SOLVER=Cfg(optim=name, lr=0.1, accum_steps=0)), params)


def test_flatten_into_cpu_fallback_adds():
    from electrocardio_panorama_amd import ops
    g = torch.Generator().manual_seed(3)
    ts = [torch.randn(5, 3, generator=g), torch.randn(7, generator=g), torch.randn(0), torch.randn(2, 2, generator=g).t()]
    cat = torch.cat([t.reshape(-1) for t in ts])
    out = torch.full((cat.numel(),), float("nan"))
    assert ops.flatten_into(ts, out) is out and torch.equal(out, cat)              # the default call assigns, as before
    base = torch.randn(cat.numel(), generator=g)
    out = base.clone()
    ops.flatten_into(ts, out, accumulate=True)
    assert torch.equal(out, base + cat)
    out = base.clone()
    ops.flatten_into(ts, out, accumulate=False)
    assert torch.equal(out, cat)
    # the word decides where it is given
    out = base.clone()
    ops.flatten_into(ts, out, accumulate=False, accumulate_dev=torch.ones(1, dtype=torch.int32))
    assert torch.equal(out, base + cat)
    out = base.clone()
    ops.flatten_into(ts, out, accumulate=True, accumulate_dev=torch.zeros(1, dtype=torch.int32))
    assert torch.equal(out, cat)
