"""Live extents, the part that needs no GPU: the new entry points are declared, bound and exported, and they changed
neither the ABI number nor the size of a kernel-argument struct; the extent rule itself against brute force."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nef_live_extent", "nef_conv_fwd_live", "nef_conv_bwd_weight_live")


def test_live_entries_declared_bound_exported():
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    build.build(verbose=False)
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    declared = set(re.findall(r"\b(nef_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    L = _lib.load()
    assert L.nef_abi_version() == 22
    assert ctypes.sizeof(_lib.ConvArgs) == 384 == L.nef_conv_args_bytes()
    assert ctypes.sizeof(_lib.BwwArgs) == 200 == L.nef_bww_args_bytes()
    # argument checks run in front of any device call
    assert L.nef_live_extent(None, None, 1, 1, 512, None) == -2
    assert L.nef_conv_fwd_live(ctypes.byref(_lib.ConvArgs()), None, 0, None) == -2
    assert L.nef_conv_bwd_weight_live(ctypes.byref(_lib.BwwArgs()), None, 0, None) == -2
    # the item tables live behind the partial sums: the workspace size counts them in, the plain entry does not need them
    w = _lib.BwwArgs(x=8, gy=8, gw=8, ws=8, B=2, T=128, G=3, Cin_g=128, Cout_g=128, K=3, form=3)
    need = L.nef_conv_bwd_weight_ws_bytes(ctypes.byref(w))
    tables = 3 * (2 * 2 * 2 + 1) * 4
    assert need > tables and (need - tables) % (3 * 3 * 128 * 128 * 4) == 0
    w.ws_bytes = need - 1
    assert L.nef_conv_bwd_weight_live(ctypes.byref(w), 8, 0, None) == -3      # NEF_E_WORKSPACE
    w.form = 0
    assert L.nef_conv_bwd_weight_live(ctypes.byref(w), 8, 0, None) == -4      # NEF_E_UNSUPPORTED: form 3 only


def live_rule(e, L):
    """nef_live_extent's rule (include/nefnet_hip.h): e = 1 + index of the last non-zero input sample."""
    cj = min(L // 2, (e + 6) // 2 + 1) if e else 0
    return min(L // 4, cj // 2 + 1) if cj else 0


def test_live_rule_is_exact():
    """Brute force over every extent of a few lengths: which conv outputs (x[2j-7 .. 2j+7]) and pooled outputs (j = 2t-1 .. 2t+1) can
    see a non-zero sample.  The rule is that set's size exactly -- never too small (which would be wrong), never too large."""
    for L in (8, 16, 20, 100, 512):
        for e in range(0, L + 1):
            x = np.zeros(L, bool)
            x[:e] = True
            c = np.array([x[max(0, 2 * j - 7):2 * j + 8].any() for j in range(L // 2)])
            p = np.array([c[max(0, 2 * t - 1):2 * t + 2].any() for t in range(L // 4)])
            want = int(np.nonzero(p)[0].max()) + 1 if p.any() else 0
            assert live_rule(e, L) == want, (L, e, live_rule(e, L), want)
