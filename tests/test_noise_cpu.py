"""CPU: the C-ABI entries of the loss with cfg.DATA.noise's addend, and the graphed step's constructor (no GPU work)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FWD_TAIL = (0.5, 0.5, 1.0, 0, 7, None)       # f0, f1, f2, reg_l2, use_mask, stream


def test_noise_entries_are_declared_bound_and_exported():
    from electrocardio_panorama_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nef_loss_noise_fwd", "nef_loss_noise_bwd"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name) and hasattr(_lib.load(), name)
    # additive: the entries without noise keep their signatures, the ABI number stays
    assert len(_lib.SIGNATURES["nef_loss_noise_fwd"][1]) == len(_lib.SIGNATURES["nef_loss_fwd"][1]) + 1
    assert len(_lib.SIGNATURES["nef_loss_noise_bwd"][1]) == len(_lib.SIGNATURES["nef_loss_bwd"][1]) + 1
    assert _lib.load().nef_abi_version() == 22      # (21 then; 22 since the single-operand packing entries went)


def test_nef_loss_noise_rejects_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the first launch, so the (non-NULL, never dereferenced) addresses below are not read.  A null
    `noise` is a legal argument: it is not what a call is refused for."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    n = L.nef_loss_ws_bytes()
    assert n > 0
    assert L.nef_loss_noise_fwd(None, 64, 64, 64, 64, 64, 64, n, 16, *FWD_TAIL) == -2        # NEF_E_NULL: pred
    assert L.nef_loss_noise_fwd(64, 64, 64, 64, 64, 64, 64, n, 0, *FWD_TAIL) == -1           # NEF_E_SHAPE: n = 0
    assert L.nef_loss_noise_fwd(64, 64, 64, 64, 64, 64, 64, 0, 16, *FWD_TAIL) == -3          # NEF_E_WORKSPACE
    assert L.nef_loss_noise_fwd(64, 64, 64, 64, None, 64, 64, n, 0, *FWD_TAIL) == -1         # null noise: the shape check is reached
    assert L.nef_loss_noise_bwd(None, 64, 64, 64, 64, None, 64, 64, 64, 16, *FWD_TAIL) == -2
    assert L.nef_loss_noise_bwd(64, 64, 64, 64, None, None, 64, 64, 64, 0, *FWD_TAIL) == -1
    # the entries without noise are the same code with noise = NULL
    assert L.nef_loss_fwd(None, 64, 64, 64, 64, 64, n, 16, *FWD_TAIL) == -2
    assert L.nef_loss_fwd(64, 64, 64, 64, 64, 64, n, 0, *FWD_TAIL) == -1
    assert L.nef_loss_fwd(64, 64, 64, 64, 64, 64, 0, 16, *FWD_TAIL) == -3
    assert L.nef_loss_bwd(64, 64, 64, 64, None, 64, 64, 64, 0, *FWD_TAIL) == -1


def test_graphed_step_constructs_with_data_noise():
    """cfg.DATA.noise no longer keeps a train step out of the captured graph: the stepper constructs (nothing touches a device before
    the first call) and knows that its slots carry a noise buffer."""
    from electrocardio_panorama_amd.graph import GraphedTrainStep
    from electrocardio_panorama_amd.network import build_model
    from test_model_gpu import make_cfg
    cfg = make_cfg(3, noise=True)
    step = GraphedTrainStep(build_model(cfg).float(), cfg)
    assert step.use_noise and step.slots == {}
    assert not GraphedTrainStep(build_model(make_cfg(3)).float(), make_cfg(3)).use_noise
