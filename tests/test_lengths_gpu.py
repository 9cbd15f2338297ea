"""Odd and short latent lengths T = L / 4 against the fp64 oracle, kernel by kernel and through the whole step.

A large share of the HIP code picks its kernel form from T alone (stem weight gradient: matrix cores only for an even T whose input
row fits in LDS; head mixes: row pairs / position pairs / scalar; every split-fp16 and Winograd conv: even T plus a size floor;
the shared decoder head: 2T >= 128).  The other GPU tests use L in {512, 520, 1000, 2048, 5000}: T even, rows short.  Here:
the stem at every tile and dispatch edge, the two-pass mixes at odd T, and the train step / eval sweep / graph replay at odd T, at
the shared-head boundary and at rows of one to sixteen positions."""
import functools
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from decisions import FLAT_TOL, TENSOR_TOL, gpu_decisions
from util import FWD_TOL, GRAD_TOL, maxabs, rel, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"

from test_model_gpu import _train_once, batch_t, conv_path, hashed_model, make_cfg, oracle_replaying  # noqa: E402,F401
from test_pano_gpu import HALF_TOL  # noqa: E402


def ops():
    from electrocardio_panorama_amd import ops as o
    return o


def g(t):
    return t.to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ 1. stem
# csrc/stem.hip: the forward tile is 63 pooled outputs (one left halo lane), the VALU weight gradient's 62 (a halo lane per side) with
# 64 partial slots walked by a strided, register-prefetched unit loop, the matrix-core weight gradient's 16 with 256 row slots.
STEM_MFMA, STEM_VALU = "stem_bwd_weight_mfma_kernel", "stem_bwd_weight_kernel"


def stem_bwd_kernel(L):
    """nef_stem_bwd_weight's rule: the matrix cores when T is even and the zero-haloed row (16 + L + 96 floats) fits in 64 KiB."""
    return STEM_MFMA if (L // 4) % 2 == 0 and (16 + L + 96) * 4 <= 64 * 1024 else STEM_VALU


# (B, V, L, seed, kernel the rule selects); seeds chosen on the CPU for the tie precondition of stem_reference
STEM_CASES = [
    (2, 3, 500, 1456, STEM_VALU),        # T = 125, odd: three tiles of 62
    (2, 1, 252, 1003, STEM_VALU),        # T = 63: one forward tile exactly, two backward tiles
    (2, 1, 244, 1003, STEM_VALU),        # T = 61: just under one backward tile
    (2, 2, 508, 1005, STEM_VALU),        # T = 127
    (70, 1, 12, 1000, STEM_VALU),        # T = 3; 70 units > 64 slots: the unit loop and its prefetch take a second trip
    (3, 2, 4, 1000, STEM_VALU),          # T = 1: the only output has no left pool neighbour
    (2, 1, 8, 1000, STEM_MFMA),          # T = 2: one ragged 16-output tile
    (1, 1, 16400, 1134, STEM_VALU),      # T = 4100, even, but the row does not fit in LDS: 67 tiles > 64 slots
    (258, 1, 8, 1011, STEM_MFMA),        # B > 256 row slots: two slots take two rows
    (1, 1, 16272, 1134, STEM_MFMA),      # the longest row the matrix-core kernel takes
]
TIE_MARGIN = 1e-5       # smallest decision margin of a case, relative to its largest conv value
# |fl(15-term fmaf chain) - exact| <= 15 * 2^-24 * sum |w_k| |x_k|, whatever the order of the taps (both weight-gradient kernels and
# the forward recompute the conv values as such chains): a decision whose margin exceeds twice that cannot fall the other way in fp32
FMA15 = 15 * 2.0 ** -24
# Rows of 4100 outputs x 128 channels hold 5e5 decisions each: over 300 seeds their smallest margin is 3.2e-7 of the largest conv
# value on average and 1.9e-6 at best (exponentially distributed: a seed with 1e-5 is one in e^31), so no seed gives them TIE_MARGIN.
# They are held to the rounding bound itself, decision by decision, with the factor 2 above; every other case to both.
LONG_ROWS = (16400, 16272)


@functools.lru_cache(maxsize=None)
def stem_reference(B, V, L, seed, grads=True):
    """fp64 on the CPU: max_pool(relu(conv)), autograd's weight gradient, the per-element sum |w_k| |x_k| the forward error is
    measured in, and the case's smallest decision margin: over every pooled output, the gap between the best and the second-best
    rectified candidate where both are positive, and the distance from 0 of the largest candidate (the selected pre-activation
    where the output is positive, the one nearest to switching on where it is not) -- as a number, and (`margin_in_bounds`) as the
    smallest ratio of an output's margin to the fp32 rounding bound of its own candidates."""
    x, w = rnd(B, V, L, seed=seed).abs(), rnd(128 * V, 1, 15, seed=seed + 1, scale=0.3)
    wr = w.double().requires_grad_(True)
    conv = F.conv1d(x.double(), wr, None, 2, 7, 1, V)
    ref = F.max_pool1d(F.relu(conv), 3, 2, 1)
    T = L // 4
    with torch.no_grad():
        bound = F.max_pool1d(F.conv1d(x.double(), w.double().abs(), None, 2, 7, 1, V), 3, 2, 1)      # x >= 0
        cand = F.pad(conv, (1, 1), value=float("-inf")).unfold(2, 3, 2)                              # [B, 128V, T, 3]: j = 2tp-1 .. 2tp+1
        assert cand.shape == (B, 128 * V, T, 3)
        top = cand.clamp(min=0).topk(2, dim=3).values
        both = top[..., 1] > 0
        gap = torch.where(both, top[..., 0] - top[..., 1], torch.full_like(bound, float("inf")))
        dist = torch.minimum(gap, cand.max(3).values.abs())                                          # each output's own margin
        out = {"x": x, "w": w, "ref": ref.detach(), "bound": bound, "margin": float(dist.min()), "cmax": float(conv.abs().max()),
               "margin_in_bounds": float((dist / (FMA15 * bound)).min())}
    if grads:
        gy = rnd(*ref.shape, seed=seed + 2)
        ref.backward(gy.double())
        out["gy"], out["gw"] = gy, wr.grad
    return out


@pytest.mark.parametrize("B,V,L,seed,kernel", STEM_CASES, ids=[f"B{c[0]}-V{c[1]}-L{c[2]}" for c in STEM_CASES])
def test_stem_lengths(B, V, L, seed, kernel):
    """Forward: rel-L2 and EVERY element within 4 eps_fp32 sum |w_k| |x_k| (one wrong halo column shows).  Weight gradient: rel-L2 of
    the whole tensor and of each lead's [128, 15] block (a lead that reads another lead's rows cannot hide)."""
    o = ops()
    assert stem_bwd_kernel(L) == kernel
    r = stem_reference(B, V, L, seed)
    # precondition, from the reference alone: no pool arg-max or ReLU decision within fp32 rounding of a tie
    assert r["margin_in_bounds"] >= 2.0, r["margin_in_bounds"]
    assert L in LONG_ROWS or r["margin"] >= TIE_MARGIN * r["cmax"], (r["margin"], r["cmax"])
    y = o.stem_fwd(g(r["x"]), g(r["w"]))
    assert y.shape == r["ref"].shape == (B, 128 * V, L // 4)
    err = (y.double().cpu() - r["ref"]).abs()
    eps = float(torch.finfo(torch.float32).eps)
    print(f"stem {(B, V, L)}: fwd rel {rel(y, r['ref']):.2e}, worst element {float((err / r['bound']).max()) / eps:.2f} eps sum|w||x|")
    assert rel(y, r["ref"]) < FWD_TOL
    assert bool((err <= 4 * eps * r["bound"]).all()), float((err / r["bound"]).max()) / eps
    gw = o.stem_bwd_weight(g(r["x"]), g(r["w"]), g(r["gy"]))
    print(f"stem {(B, V, L)}: gw rel {rel(gw, r['gw']):.2e} ({kernel})")
    assert rel(gw, r["gw"]) < GRAD_TOL
    for v in range(V):
        blk = slice(128 * v, 128 * (v + 1))
        assert rel(gw[blk], r["gw"][blk]) < GRAD_TOL, (v, rel(gw[blk], r["gw"][blk]))


def test_stem_cases_reach_every_backward_kernel():
    """The cases above launch both weight-gradient kernels and, through each, the reduction of their partial slots; the row-slot loop of
    the matrix-core kernel (B > 256) and the second trip of the VALU kernel's unit loop (units > 64) are among them."""
    assert {c[4] for c in STEM_CASES} == {STEM_MFMA, STEM_VALU}
    assert any(c[4] == STEM_MFMA and c[0] > 256 for c in STEM_CASES)
    assert any(c[4] == STEM_VALU and c[0] * -(-(c[2] // 4) // 62) > 64 for c in STEM_CASES)
    assert stem_bwd_kernel(16272) == STEM_MFMA and stem_bwd_kernel(16276) == STEM_VALU


# ------------------------------------------------------------------------------------------------ 2. the two-pass mixes at odd T
@pytest.mark.parametrize("T", [1, 3, 125])
def test_two_pass_mixes_at_odd_lengths(T):
    """lead_mean, mix_fwd, mix_bwd and mix_bwd(upsampled=True) -- the non-shared head of rows shorter than 64 -- against test_mix's
    restatement in fp64, at its bars (1e-6 forward, 1e-5 gradients)."""
    o = ops()
    from oracle import nefnet_oracle as orc
    B, V, c1, c2 = 3, 3, 2, 1
    z1f, z2f, qf = rnd(B, 128 * V, T, seed=232), rnd(B, 128 * V, T, seed=233), rnd(B, 256, seed=234)

    def restate():
        z1, z2r, q = (t.double().requires_grad_(True) for t in (z1f, z2f, qf))
        z1m, z2m = orc.lead_mean(z1, V), orc.lead_mean(z2r, V)
        latent = torch.cat([z1m, z2m], 1)
        D = torch.cat([q[:, :, None] * latent,
                       q[:, :, None] * torch.cat([z1[:, 128 * c1:128 * (c1 + 1)], z2m], 1),
                       q[:, :, None] * torch.cat([z1m, z2r[:, 128 * c2:128 * (c2 + 1)]], 1)], 0)
        return z1, z2r, q, latent, D

    z1, z2r, q, latent, D = restate()
    lat_d = o.lead_mean(g(z1f), g(z2f), V)
    assert rel(lat_d, latent) < 1e-6
    Dd = o.mix_fwd(lat_d, g(z1f), g(z2f), g(qf), V, c1, c2)
    assert rel(Dd, D) < 1e-6
    gD = rnd(*D.shape, seed=235)
    D.backward(gD.double())
    for relu in (False, True):
        gz1, gz2r, gq = o.mix_bwd(g(gD), lat_d, g(z1f), g(z2f), g(qf), V, c1, c2, relu_z1=relu)
        want1 = z1.grad * (z1f > 0) if relu else z1.grad
        assert rel(gz1, want1) < 1e-5 and rel(gz2r, z2r.grad) < 1e-5 and rel(gq, q.grad) < 1e-5, (T, relu)
    # the gradient wrt the x2-upsampled decoder input: the adjoint is taken while reading (at T = 1 both positions are edges)
    z1, z2r, q, latent, D = restate()
    gU = rnd(3 * B, 256, 2 * T, seed=236)
    F.interpolate(D, scale_factor=2, mode="linear", align_corners=False).backward(gU.double())
    gz1, gz2r, gq = o.mix_bwd(g(gU), lat_d, g(z1f), g(z2f), g(qf), V, c1, c2, upsampled=True)
    assert rel(gz1, z1.grad) < 1e-5 and rel(gz2r, z2r.grad) < 1e-5 and rel(gq, q.grad) < 1e-5, T


# ------------------------------------------------------------------------------------------------ 3. whole step, sweep, replay
# (B, V, L)
TRAIN_CASES = [
    (2, 3, 500),       # T = 125, odd: shared head, scalar un-pooling mixes, VALU stem gradient, direct fp32 convs
    (2, 3, 508),       # T = 127
    (2, 3, 260),       # T = 65: just above the shared-head boundary
    (2, 1, 252),       # T = 63: just below it, and odd
    (2, 8, 256),       # T = 64: exactly on it
    (4, 3, 36),        # T = 9
    (2, 3, 64),        # T = 16: packed short-row split-fp16 convs
    (4, 1, 12),        # T = 3
    (2, 1, 8),         # T = 2
    (2, 1, 4),         # T = 1
]
SEEDS = (31, 32)
LENGTH_FACTS = {}      # (conv path, B, V, L, seed, masked) -> (flat, worst tensor rel, its name, outputs rel, replayed ties)


def _report_lengths():
    """One line in the run's `---- parity facts ----` tail (latest state: the line is replaced, not repeated)."""
    import conftest
    tag = "odd / short lengths:"
    flat = max(LENGTH_FACTS.items(), key=lambda kv: kv[1][0])
    tens = max(LENGTH_FACTS.items(), key=lambda kv: kv[1][1])
    outs = max(LENGTH_FACTS.items(), key=lambda kv: kv[1][3])
    conftest.REPORT[:] = [l for l in conftest.REPORT if not l.startswith(tag)]
    conftest.report(f"{tag} {len(LENGTH_FACTS)} train steps vs the replaying fp64 oracle, worst flat gradient {flat[1][0]:.2e} <= {FLAT_TOL:g} "
                    f"{flat[0]}, worst tensor {tens[1][1]:.2e} <= {TENSOR_TOL:g} ({tens[1][2]}, {tens[0]}), worst output "
                    f"{outs[1][3]:.2e} <= {FWD_TOL:g} {outs[0]}, {sum(v[4] for v in LENGTH_FACTS.values())} replayed tie(s)")


ZERO_SUM_FACTS = {}      # (conv path, seed) -> (name, the oracle's own fp32 residue) of the largest measured floor at L = 4


def _zero_sum_floor(m, outs, b, V, seed):
    """L = 4: the first decoder BatchNorm normalises four values per channel and pass (B = 2 rows of 2 positions), its invstd reaches
    1 / sqrt(1e-5) and the terms of the analytically zero conv-bias gradients in front of it are of size 10 where the BatchNorm-bias
    gradient that assert_grad_parity scales their absolute bar by is 0.02: round-off of a correct fp32 sum misses 1e-6 (measured:
    1.25e-6 on decoder.1.double_conv.0.bias, split-fp16 path, seed 32; the oracle's own fp32 run leaves 6.3e-7 there and its fp64 run
    1.7e-15 = 2^-53 x 15).  So the bar is measured, not widened by eye: the oracle's own fp32 residue of the same sum at this shape and
    seed, replaying the same decisions, times 4 for the different summation order of a tiled kernel."""
    from oracle import hashweights as hw
    from oracle import nefnet_oracle as orc
    dec = orc.Decisions(gpu_decisions(m, outs, b["target_view"].unsqueeze(1), keep_masks=None, reg_l1=True))
    P = orc.require_grad(hw.hashed_params(V))
    random.seed(seed)
    ref = orc.forward(P, hw.hashed_buffers(), b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train", training=True,
                      masks=None, p=0.0, dec=dec)
    orc.loss_v1(ref[0], ref[1], ref[2], b["target_view"].unsqueeze(1), reg_loss="l1_loss", dec=dec)[0].backward()
    own = {k: float(v.grad.abs().max()) for k, v in P.items() if k.endswith("double_conv.0.bias") or k.endswith("double_conv.3.bias")}
    return {k: 4 * v for k, v in own.items()}, max(own.items(), key=lambda kv: kv[1])


def _step_vs_oracle(path, B, V, L, seed, masked):
    from oracle import hashweights as hw
    from oracle import nefnet_oracle as orc
    from electrocardio_panorama_amd import engine
    T = L // 4
    assert engine._head_shared(T) == (T >= 64)
    m, outs, losses = _train_once(V, B, L, seed, "l1_loss", masked)
    assert all(a.shape == (B, 1, L) for a in outs) and m.segment_status() == 0
    masks = hw.hashed_masks(V, B, T) if masked else None
    host, floor = batch_t(B, V, L, seed, dev="cpu"), None
    if L == 4 and not masked:
        import conftest
        floor, ZERO_SUM_FACTS[(path, seed)] = _zero_sum_floor(m, outs, host, V, seed)
        tag, worst = "L = 4, analytically zero conv-bias gradients:", max(ZERO_SUM_FACTS.items(), key=lambda kv: kv[1][1])
        conftest.REPORT[:] = [l for l in conftest.REPORT if not l.startswith(tag)]
        conftest.report(f"{tag} absolute bar = max(1e-6, 4 x the oracle's own fp32 residue); largest residue {worst[1][1]:.2e} "
                        f"({worst[1][0]}, {worst[0]})")
    ref, rl, dec, flat = oracle_replaying(m, outs, host, V, seed, masks=masks, dt=torch.float64, zero_floor=floor)
    o_rel = max(rel(a, r) for a, r in zip(outs, ref))
    assert o_rel < FWD_TOL, o_rel
    assert maxabs(torch.stack([l_.detach() for l_ in losses]), torch.stack([r.detach() for r in rl])) < 1e-6
    assert flat < FLAT_TOL
    worst = (0.0, None)
    for k, p in m.named_parameters():
        if k in orc.DEAD_PARAMS or k.endswith("double_conv.0.bias") or k.endswith("double_conv.3.bias"):
            continue      # (no gradient / analytically zero: held to an absolute bar inside oracle_replaying)
        e = rel(p.grad, dec.oracle_params[k].grad)
        if e > worst[0]:
            worst = (e, k)
    assert worst[0] < TENSOR_TOL, worst
    LENGTH_FACTS[(path, B, V, L, seed, masked)] = (flat, worst[0], worst[1], o_rel, dec.total_flips())
    print(f"lengths {(path, B, V, L, seed, masked)}: flat {flat:.2e}, worst tensor {worst[0]:.2e} {worst[1]}, outputs {o_rel:.2e}, "
          f"{dec.total_flips()} replayed tie(s)")
    _report_lengths()


@pytest.mark.parametrize("B,V,L", TRAIN_CASES, ids=[f"B{c[0]}-V{c[1]}-L{c[2]}" for c in TRAIN_CASES])
def test_train_step_lengths_vs_oracle(conv_path, B, V, L):
    """Outputs at FWD_TOL, losses at 1e-6, the flat and every tensor's gradient at the tie-free bars against the fp64 oracle that
    replays the step's decisions, every replayed decision certified as a tie; two seeds per shape, dropout off."""
    for seed in SEEDS:
        _step_vs_oracle(conv_path, B, V, L, seed, False)


def test_train_step_odd_length_with_dropout_masks(conv_path):
    """T = 125 with the hashed dropout masks replayed on both sides."""
    for seed in SEEDS:
        _step_vs_oracle(conv_path, 2, 3, 500, seed, True)


@pytest.mark.parametrize("B,V,L", [(2, 3, 500), (2, 1, 36)])
def test_eval_sweep_lengths_vs_oracle(B, V, L):
    """phase='test' with five queried angles against the oracle's eval forward; gen_ecg gives the sweep's own bits; the fp16 decoder
    within the half-precision gate of both."""
    from oracle import hashweights as hw
    from oracle import nefnet_oracle as orc
    Q, seed = 5, 41
    b = batch_t(B, V, L, seed, Q, dev="cpu")
    bd = {k: v.to(DEV) for k, v in b.items()}
    m = hashed_model(V).eval()
    random.seed(seed)
    outs = m(bd["data"], bd["input_theta"], bd["target_theta"], bd["rois"], rest_theta=bd["rest_theta"], phase="test")
    with torch.no_grad():
        random.seed(seed)
        ref = orc.forward(hw.hashed_params(V), hw.hashed_buffers(), b["data"], b["input_theta"], b["target_theta"], b["rois"],
                          rest_theta=b["rest_theta"], phase="test", training=False)
    assert outs[3].shape == (B, Q, L)
    for a, r in zip(outs, ref):
        assert rel(a, r) < FWD_TOL, rel(a, r)
    z1, z2 = m(bd["data"], bd["input_theta"], bd["target_theta"], bd["rois"], phase="gen")
    assert z1.shape == (B, 128 * V, L // 4) and m.segment_status() == 0
    assert rel(m.gen_ecg(z1, z2, bd["rest_theta"], bd["rois"]), ref[3]) < FWD_TOL
    m.panorama_dtype = "fp16"
    random.seed(seed)
    half = m(bd["data"], bd["input_theta"], bd["target_theta"], bd["rois"], rest_theta=bd["rest_theta"], phase="test")
    for a, r in zip(half[:3], outs[:3]):
        assert torch.equal(a, r)
    assert half[3].shape == (B, Q, L) and rel(half[3], ref[3]) < HALF_TOL, rel(half[3], ref[3])
    assert rel(m.gen_ecg(z1, z2, bd["rest_theta"], bd["rois"]), ref[3]) < HALF_TOL


@pytest.mark.parametrize("B,V,L", [(2, 3, 500), (4, 1, 12)])
def test_graph_replay_lengths_equal_eager(B, V, L):
    """Three replayed train steps against three eager Solver steps, dropout off: losses and every parameter bit for bit."""
    from electrocardio_panorama_amd import synth
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    batches = [synth.make_batch(B, V, L, seed=60 + s, Q=2) for s in range(3)]
    got = {}
    for graph in (False, True):
        cfg = make_cfg(V)
        cfg.SOLVER["graph"] = graph
        sol = Solver(cfg, use_tensorboardx=False)
        sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
        sol.model.dropout_p = 0.0
        opt = get_optimizer(cfg, sol.model.parameters())
        random.seed(17)
        losses = sol.run_one_epoch(batches, "train", opt, collect_views=False)[0]
        st = getattr(sol, "_graph_stepper", None)
        assert (st is not None) == graph
        if graph:
            assert st.calls == 3 and len(st.slots) == 1
        got[graph] = (np.array(losses), {k: v.clone() for k, v in sol.model.state_dict().items()})
    assert got[True][0].shape[0] == 3 and np.array_equal(got[False][0], got[True][0]), (got[False][0], got[True][0])
    for k, v in got[False][1].items():
        assert torch.equal(v, got[True][1][k]), k


def test_signal_length_contract(monkeypatch):
    """Every multiple of 4 from MIN_SIGNAL_LENGTH = 4 up runs (TRAIN_CASES holds L = 4 and L = 8 to the oracle); anything else is a
    ValueError that names the minimum, raised before the first launch -- by the model and by the graphed step -- and README.md states the
    minimum once."""
    import os
    from electrocardio_panorama_amd import ops as o
    from electrocardio_panorama_amd.graph import GraphedTrainStep
    from electrocardio_panorama_amd.network.model_nefnet import MIN_SIGNAL_LENGTH
    assert MIN_SIGNAL_LENGTH == 4 == min(c[2] for c in TRAIN_CASES)
    readme = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md")).read()
    assert readme.count("MIN_SIGNAL_LENGTH") == 1 and f"`MIN_SIGNAL_LENGTH = {MIN_SIGNAL_LENGTH}`" in readme
    m = hashed_model(1).train()
    step = GraphedTrainStep(m, make_cfg(1))

    def launched(*a, **k):
        raise AssertionError("a launch before the length check")
    monkeypatch.setattr(o, "pack_many", launched)
    monkeypatch.setattr(o, "stem_fwd", launched)
    b = batch_t(2, 1, 8, 3)
    for L in (0, 2, 6, 10):
        x = torch.zeros(2, 1, L, device=DEV)
        for phase in ("train", "test", "gen"):
            with pytest.raises(ValueError, match=f"multiple of 4, at least {MIN_SIGNAL_LENGTH}"):
                m(x, b["input_theta"], b["target_theta"], b["rois"], rest_theta=b["target_theta"].unsqueeze(1), phase=phase)
        with pytest.raises(ValueError, match=f"multiple of 4, at least {MIN_SIGNAL_LENGTH}"):
            step(x, b["input_theta"], b["target_theta"], b["rois"], torch.zeros(2, L, device=DEV))
