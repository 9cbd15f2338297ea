"""CPU: layer-wise trust ratios (SOLVER.optim lars / lamb) -- the nef_update_trust C-ABI entry, the segment table and the Python surface
(no GPU work)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DECAY = ["*.bias", "decoder.*.double_conv.[14].weight"]      # the model's 1-D tensors


class Cfg(dict):
    __getattr__ = dict.__getitem__


def test_header_declares_the_entries_and_binding_has_them():
    from electrocardio_panorama_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    assert re.search(r"\bint nef_update_trust\s*\(\s*const nef_update_args\s*\*\s*a,\s*const nef_trust_args\s*\*\s*t,\s*const nef_ema_args\s*\*", hdr)
    assert re.search(r"\bsize_t nef_update_trust_ws_bytes\s*\(\s*int64_t n,\s*int32_t n_segs\)", hdr)
    assert re.search(r"\bsize_t nef_trust_args_bytes\s*\(\s*void\s*\)", hdr)
    assert re.search(r"typedef struct nef_trust_args\s*\{", hdr) and re.search(r"\}\s*nef_trust_args\s*;", hdr)
    assert re.search(r"#define NEF_TRUST_MAX_SEGS 256\b", hdr)
    assert "THE SEGMENT TABLE IS THE CALLER'S DUTY" in hdr
    L = _lib.load()
    for name in ("nef_update_trust", "nef_update_trust_ws_bytes", "nef_trust_args_bytes"):
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
    assert ctypes.sizeof(_lib.TrustArgs) == L.nef_trust_args_bytes()
    # additive: the ABI number, nef_update's struct and its rule set are what they were
    assert L.nef_abi_version() == 22
    assert ctypes.sizeof(_lib.UpdateArgs) == 144 == L.nef_update_args_bytes()
    a = _lib.UpdateArgs(p=64, g=64, buf=64, m=64, v=64, step=64, n=16, lr=0.1, gscale=1.0, mu=0.9, beta1=0.9, beta2=0.999, eps=1e-8, rule=3)
    assert L.nef_update(ctypes.byref(a), None) == -4


def test_workspace_depends_on_n_and_the_segment_count_alone():
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    w = L.nef_update_trust_ws_bytes
    assert w(1, 1) > 0 and w(0, 1) == 0 and w(16, 0) == 0
    assert w(16, 2) - w(16, 1) == 16                      # one fp64 pair per segment more
    assert w(1 << 24, 53) > w(1 << 20, 53) >= 2 * 8 * 53
    assert w(7_180_000, 53) < 64 * 1024                   # the partials of the flagship's parameters stay in a few KiB


def _call(a_kw=None, t_kw=None, t_null=False):
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    a = _lib.UpdateArgs(p=64, g=64, buf=64, m=64, v=64, step=64, n=16, lr=0.1, gscale=1.0, mu=0.9, beta1=0.9, beta2=0.999, eps=1e-6)
    t = _lib.TrustArgs(seg_end=64, seg_wd_mul=64, seg_adapt=64, ratio=64, stats=64, taint=None, ws=64, ws_bytes=1 << 20,
                       trust_coef=1e-3, trust_eps=1e-8, n_segs=2)
    for k, v in (a_kw or {}).items():
        setattr(a, k, v)
    for k, v in (t_kw or {}).items():
        setattr(t, k, v)
    return L.nef_update_trust(ctypes.byref(a), None if t_null else ctypes.byref(t), None, None)


def test_nef_update_trust_rejects_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the first launch, so the (non-NULL, never dereferenced) addresses are not read."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    assert L.nef_update_trust(None, None, None, None) == -2                   # NEF_E_NULL
    assert _call(t_null=True) == -2
    for k in ("seg_end", "seg_wd_mul", "seg_adapt", "ratio", "stats", "ws"):
        for rule in (0, 1):
            assert _call({"rule": rule}, {k: None}) == -2, k
    assert _call({"p": None}) == -2 and _call({"g": None}) == -2
    assert _call({"rule": 0, "buf": None}) == -2
    for k in ("m", "v", "step"):
        assert _call({"rule": 1, k: None}) == -2
    for rule in (0, 1):
        assert _call({"rule": rule}, {"n_segs": 0}) == -1                     # NEF_E_SHAPE
        assert _call({"rule": rule}, {"n_segs": 257}) == -1
        assert _call({"rule": rule, "n_runs": 1, "run_end": 64, "run_mul": 64}) == -1      # the multipliers travel per segment
        assert _call({"rule": rule, "n": 0}) == -1
        assert _call({"rule": rule, "weight_decay": -0.1}) == -1
        assert _call({"rule": rule}, {"trust_coef": -1e-3}) == -1
        assert _call({"rule": rule}, {"trust_eps": -1e-8}) == -1
        assert _call({"rule": rule}, {"trust_coef": float("nan")}) == -1
        need = L.nef_update_trust_ws_bytes(16, 2)
        assert _call({"rule": rule}, {"ws_bytes": need - 1}) == -3            # NEF_E_WORKSPACE
        assert _call({"rule": rule}, {"ws_bytes": 0}) == -3
    assert _call({"rule": 2}) == -4                                           # NEF_E_UNSUPPORTED: AdamW has no trust-ratio form
    assert _call({"rule": 3}) == -4 and _call({"rule": -1}) == -4


def test_trust_segments():
    from electrocardio_panorama_amd.solver.optim_scheduler import trust_segments
    names = ["a.weight", "a.bias", "b.weight", "b.bias", "decoder.4.bias"]
    sizes = [12, 3, 20, 5, 1]
    ends = [12, 15, 35, 40, 41]
    assert trust_segments(names, sizes, (), ()) == (ends, [1.0] * 5, [1.0] * 5)
    # one segment per tensor: neighbours with equal numbers do NOT merge (a ratio belongs to one tensor)
    assert trust_segments(names, sizes, ["*.bias"], ()) == (ends, [1.0, 0.0, 1.0, 0.0, 0.0], [1.0] * 5)
    assert trust_segments(names, sizes, (), ["*.bias"]) == (ends, [1.0] * 5, [1.0, 0.0, 1.0, 0.0, 0.0])
    assert trust_segments(names, sizes, ["a.*"], ["decoder.4.bias", "b.weight"]) == (ends, [0.0, 0.0, 1.0, 1.0, 1.0], [1.0, 1.0, 0.0, 1.0, 0.0])
    assert trust_segments(names, sizes, ["*"], ["*"]) == (ends, [0.0] * 5, [0.0] * 5)
    # an unnamed tensor is never exempt, from either
    assert trust_segments([None, "x.bias"], [4, 2], ["*"], ["*"]) == ([4, 6], [1.0, 0.0], [1.0, 0.0])
    # an empty tensor makes no segment
    assert trust_segments(["w", "e.bias", "z.bias"], [4, 0, 2], ["*.bias"], ["z.*"]) == ([4, 6], [1.0, 0.0], [1.0, 0.0])
    assert trust_segments(["A.Bias"], [3], ["*.bias"], ["*.bias"]) == ([3], [1.0], [1.0])      # case-sensitive


def test_trust_segments_on_the_model():
    from electrocardio_panorama_amd.config import get_defaults
    from electrocardio_panorama_amd.network import build_model
    from electrocardio_panorama_amd.solver.optim_scheduler import MAX_SEGS, trust_segments
    cfg = get_defaults()
    cfg.MODEL.model = "model_nefnet"
    cfg.DATA.lead_num = 3
    m = build_model(cfg)
    named = list(m.named_parameters())
    assert len(named) == 53 and MAX_SEGS == 256
    names, sizes = [k for k, _ in named], [p.numel() for _, p in named]
    ends, wd_muls, adapts = trust_segments(names, sizes, NO_DECAY, NO_DECAY)
    assert len(ends) == len(wd_muls) == len(adapts) == 53                        # one segment each
    off = 0
    for (k, p), e, w, a in zip(named, ends, wd_muls, adapts):
        off += p.numel()
        assert e == off, k
        assert w == a == (0.0 if p.dim() == 1 else 1.0), (k, tuple(p.shape))     # exactly the 1-D tensors are exempt
    i = names.index("decoder.4.bias")
    assert sizes[i] == 1 and ends[i] - (ends[i - 1] if i else 0) == 1            # a one-element segment


def test_config_defaults():
    from electrocardio_panorama_amd.config import get_defaults
    s = get_defaults().SOLVER
    assert s.trust_coef == 1e-3 and s.trust_eps == 1e-8 and s.trust_exempt == []
    cfg = get_defaults()
    cfg.merge_from_list(["SOLVER.optim", "lamb", "SOLVER.trust_coef", "2e-3", "SOLVER.trust_exempt", "['*.bias']"])
    assert cfg.SOLVER.optim == "lamb" and cfg.SOLVER.trust_coef == 2e-3 and cfg.SOLVER.trust_exempt == ["*.bias"]


def test_get_optimizer_maps_the_keys():
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedAdam, FusedLAMB, FusedLARS, FusedSGD, get_optimizer
    params = [torch.nn.Parameter(torch.zeros(3))]
    # configs written before the keys existed
    opt = get_optimizer(Cfg(SOLVER=Cfg(optim="lars", lr=0.1)), params)
    g = opt.param_groups[0]
    assert type(opt) is FusedLARS and isinstance(opt, FusedSGD) and opt.trust_exempt == () and opt.no_decay == ()
    assert g["trust_coef"] == 1e-3 and g["trust_eps"] == 1e-8 and g["momentum"] == 0.9 and g["weight_decay"] == 0 and g["nesterov"] is False
    opt = get_optimizer(Cfg(SOLVER=Cfg(optim="lamb", lr=1e-3)), params)
    g = opt.param_groups[0]
    assert type(opt) is FusedLAMB and isinstance(opt, FusedAdam) and opt.trust_exempt == ()
    assert g["eps"] == 1e-6 and g["weight_decay"] == 0 and g["trust_coef"] == 1e-3 and g["trust_eps"] == 1e-8
    # ... and with them
    s = Cfg(optim="lars", lr=0.1, weight_decay=0.05, nesterov=True, no_decay=["*.bias"], trust_exempt=["*.bias", "bn.*"], trust_coef=2e-3,
            trust_eps=1e-9, clip_grad_norm=0.5, ema_decay=0.99)
    opt = get_optimizer(Cfg(SOLVER=s), params)
    g = opt.param_groups[0]
    assert type(opt) is FusedLARS and g["trust_coef"] == 2e-3 and g["trust_eps"] == 1e-9 and g["weight_decay"] == 0.05 and g["nesterov"] is True
    assert opt.trust_exempt == ("*.bias", "bn.*") and opt.no_decay == ("*.bias",) and opt.max_grad_norm == 0.5 and opt.ema_decay == 0.99
    # group keys travel in the state dict; the pattern lists are attributes and do not
    sd = opt.state_dict()["param_groups"][0]
    assert sd["trust_coef"] == 2e-3 and sd["trust_eps"] == 1e-9 and "trust_exempt" not in sd and "no_decay" not in sd
    assert opt._captured_scalars(g)[-2:] == (2e-3, 1e-9)
    s["optim"] = "lamb"
    opt = get_optimizer(Cfg(SOLVER=s), params)
    g = opt.param_groups[0]
    assert type(opt) is FusedLAMB and g["weight_decay"] == 0.05 and g["trust_coef"] == 2e-3 and opt.trust_exempt == ("*.bias", "bn.*")
    assert opt._captured_scalars(g)[-2:] == (2e-3, 1e-9)
    assert opt.trust_ratios() == {} and opt.trust_stats is None                  # nothing is built before the first step


def test_validation_errors():
    from electrocardio_panorama_amd.solver.optim_scheduler import FusedLAMB, FusedLARS
    params = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (dict(trust_coef=-1e-3), dict(trust_eps=-1.0), dict(trust_coef=float("nan"))):
        with pytest.raises(ValueError):
            FusedLARS(params, lr=0.1, **bad)
        with pytest.raises(ValueError):
            FusedLAMB(params, **bad)
    with pytest.raises(ValueError):
        FusedLARS(params, lr=-0.1)
    with pytest.raises(ValueError):
        FusedLARS(params, lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(NotImplementedError):
        FusedLARS(params, lr=0.1, dampening=0.1)
    with pytest.raises(ValueError):
        FusedLAMB(params, weight_decay=-1e-3)
    with pytest.raises(NotImplementedError):
        FusedLAMB(params, amsgrad=True)
    # a pattern given as one string is one pattern
    assert FusedLARS(params, lr=0.1, trust_exempt="*.bias").trust_exempt == ("*.bias",)
    # a checkpoint written by torch's SGD / Adam (no trust keys in the group) loads: the optimiser's defaults stand in
    o = FusedLARS(params, lr=0.1, trust_coef=5e-3)
    o.load_state_dict(torch.optim.SGD(params, lr=0.1, momentum=0.9).state_dict())
    assert o._captured_scalars(o.param_groups[0])[-2:] == (5e-3, 1e-8)
    o = FusedLAMB(params)
    o.load_state_dict(torch.optim.Adam(params).state_dict())
    assert o._captured_scalars(o.param_groups[0])[-2:] == (1e-3, 1e-8)
