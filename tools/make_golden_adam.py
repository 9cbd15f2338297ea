"""Generate tests/golden/adam_B4_V3_L512.npz by running the REFERENCE's own Solver with optim='adam'.  Build-container only (CPU).

    python tools/make_golden_adam.py            (from the repo root; needs the reference checkout oracle/make_golden.py names)

Three iterations of the reference's Solver.run_one_epoch(phase='train') with its get_optimizer -> torch.optim.Adam(lr=1e-3), the hash
weights of oracle/hashweights.py and dropout 0, on synth.make_batch(4, 3, 512, seed=21 + s, Q=2): the case of oracle/make_golden.py's
sgd fixture with the other optimiser.  The fixture has the same keys as sgd_B4_V3_L512.npz (data only: seeds, losses, parameter
subsamples and statistics, buffers), plus what the GPU test needs to bound sign flips.  Adam's update of an element is about
lr * sign(m), whatever the gradient's size: an element whose reference gradient is smaller than the error of another fp32 computation
of it can move the other way.  Per parameter and step the fixture stores `grms:<name>` (the gradient's RMS) and `gsmall:<name>` (the
fraction of elements with 0 < |g| < 1e-3 x RMS; the HIP path's gradients are held to 1e-4 rel-L2 of the reference's, so this is ten
times that error level).  Exact zeros are not counted: they are structural (dead ReLU units, rows the ROI window never reads) and
give no update on either path."""
SMALL = 1e-3
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as mg            # noqa: E402  (its helpers; the module is not changed)
from oracle import hashweights as hw            # noqa: E402
from electrocardio_panorama_amd import synth    # noqa: E402


def _stub_optional_modules():
    """The optional imports of the reference's solver module, as oracle/make_golden.py's case_sgd stubs them (kept in step with it)."""
    for mod in ("tensorboardX", "skimage", "skimage.metrics", "matplotlib", "matplotlib.pyplot"):
        if mod not in sys.modules:
            try:
                __import__(mod)
            except Exception:
                sys.modules[mod] = types.ModuleType(mod)
    sk = sys.modules["skimage.metrics"]
    if not hasattr(sk, "structural_similarity"):
        sk.structural_similarity = lambda *a, **k: 0.0
        sk.peak_signal_noise_ratio = lambda *a, **k: 0.0
    if not hasattr(np, "float"):
        np.float, np.int = float, int


def case_adam(network, B, V, L, seed, steps=3, lr=1e-3):
    _stub_optional_modules()
    from solver.solver import Solver
    from solver.optim_scheduler import get_optimizer
    import solver.solver as ss
    cfg = mg.ref_cfg(V, lr=lr)
    cfg.SOLVER["optim"] = "adam"
    real_build = network.build_model
    ss.build_model = lambda c: mg.ref_model(network, V)
    try:
        sol = Solver(cfg, use_tensorboardx=False)
    finally:
        ss.build_model = real_build
    ss.tqdm = lambda x: x
    batches = []
    for s in range(steps):
        b = mg.to_t(synth.make_batch(B, V, L, seed=seed + s, Q=2))
        b["ori_data"] = b["data"]
        b["unsupervision_lead_name"] = []
        batches.append(b)
    opt = get_optimizer(cfg, sol.model.parameters())
    assert type(opt).__name__ == "Adam", type(opt)
    gstat = {}

    def record(g, k):
        g = g.detach().double()
        rms = float(g.norm()) / g.numel() ** 0.5
        a = g.abs()
        gstat.setdefault(k, []).append((rms, float(((a > 0) & (a < SMALL * rms)).double().mean()) if rms > 0 else 0.0))
        return None          # (a hook that returns a tensor REPLACES the gradient)

    hooks = [p.register_hook(lambda g, k=k: record(g, k)) for k, p in sol.model.named_parameters()]
    random.seed(seed)
    st = random.getstate()
    losses = sol.run_one_epoch(batches, "train", opt)[0]
    for h in hooks:
        h.remove()
    random.setstate(st)
    choices = [[random.randint(0, V - 1), random.randint(0, V - 1)] for _ in range(steps)]
    sd = sol.model.state_dict()
    P, Bf = hw.hashed_params(V), hw.hashed_buffers()
    save = dict(B=B, V=V, L=L, seed=seed, steps=steps, lead_choice=np.array(choices), losses=np.array(losses), lr=lr)
    for k in P:
        save["psub:" + k] = mg.sub(sd[k], 128)
        save["pstat:" + k] = mg.stats(sd[k])
    for k in Bf:
        save["buf:" + k] = sd[k].numpy()
    for k, v in gstat.items():
        assert len(v) == steps, (k, len(v))
        save["grms:" + k] = np.array([x[0] for x in v])
        save["gsmall:" + k] = np.array([x[1] for x in v])
    name = f"adam_B{B}_V{V}_L{L}"
    np.savez_compressed(os.path.join(mg.OUT, name + ".npz"), **save)
    print(f"{name}: losses {np.array(losses)[:, 0]}")


def main():
    os.makedirs(mg.OUT, exist_ok=True)
    torch.set_num_threads(8)
    case_adam(mg.import_reference(), 4, 3, 512, seed=21)


if __name__ == "__main__":
    main()
