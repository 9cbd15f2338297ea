"""Lead masks on the GPU (MODEL.lead_mask): the three entries of csrc/lead_mask.hip against the existing kernels (all-ones masks, bit
for bit) and against the numpy restatement (tests/lead_mask_ref.py) at the bounds of the defined fp32 expressions; the masked model
against the unmasked two-lead sub-model; the replayed step against the eager one, a resumed epoch, and on / off."""
import random

import numpy as np
import pytest
import torch

import lead_mask_ref as ref
from decisions import FLAT_TOL, TENSOR_TOL, assert_grad_parity
from util import FWD_TOL, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = ref.U24


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the mix kernels
# (B, V, T): every T of the list, every V, B = 1..3; odd T puts every row offset (0..3 floats behind a 16-byte boundary) in play,
# T = 1..3 are rows shorter than a vector, 64 / 65 one lane trip and one more, 130 two column groups per trip, 1250 the flagship's rows
CASES = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (3, 12, 3), (2, 12, 31), (3, 3, 64), (2, 2, 65), (2, 1, 65), (1, 12, 130), (2, 3, 130), (1, 3, 1250)]
IDS = [f"B{B}_V{V}_T{T}" for B, V, T in CASES]


def _leads(B, V, T, seed):
    rng = np.random.default_rng(seed)
    z1 = rng.standard_normal((B, 128 * V, T), dtype=np.float32)
    z2r = rng.standard_normal((B, 128 * V, T), dtype=np.float32)
    q = rng.standard_normal((B, 256), dtype=np.float32)
    return z1, z2r, q


def _mask(B, V, seed):
    """Random, every sample keeps a lead; sample 0 keeps exactly one (its last), so n_b = 1 is always among them."""
    rng = np.random.default_rng(seed)
    m = (rng.random((B, V)) < 0.5).astype(np.uint8)
    m[0] = 0
    m[0, V - 1] = 1
    for b in range(1, B):
        if not m[b].any():
            m[b, rng.integers(V)] = 1
    return m


def _fill_absent(z, mask, value):
    z = z.copy()
    B, V = mask.shape
    zz = z.reshape(B, V, 128, -1)
    zz[mask == 0] = value
    return z


@pytest.mark.parametrize("B,V,T", CASES, ids=IDS)
def test_all_ones_mask_is_the_unmasked_head_bit_for_bit(B, V, T):
    from electrocardio_panorama_amd import ops
    z1, z2r, q = (g(a) for a in _leads(B, V, T, 1))
    ones = torch.ones(B, V, dtype=torch.uint8, device=DEV)
    c = (V - 1, 0)
    latent, D, pk = ops.lead_mask_mix_fwd(z1, z2r, ones, q, c, picks=True)
    want_l = ops.lead_mean(z1, z2r, V)
    assert torch.equal(latent, want_l) and torch.equal(D, ops.mix_fwd(want_l, z1, z2r, q, V, c))
    assert pk.tolist() == [list(c)] * B
    assert torch.equal(ops.lead_mask_mix_fwd(z1, z2r, ones.bool(), q, torch.tensor(c, dtype=torch.int32, device=DEV))[1], D)
    rng = np.random.default_rng(2)
    for up in (False, True):
        gD = g(rng.standard_normal((3 * B, 256, 2 * T if up else T), dtype=np.float32))
        for relu in (False, True):
            gz1, gz2r, gq = ops.lead_mask_mix_bwd(gD, latent, z1, z2r, q, ones, c, up=up, relu_z1=relu)
            w1, w2, wq = ops.mix_bwd(gD, latent, z1, z2r, q, V, c, upsampled=up, relu_z1=relu)
            assert torch.equal(gz1, w1) and torch.equal(gz2r, w2), (up, relu)
            r = ref.backward(gD.cpu().numpy(), latent.cpu().numpy(), z1.cpu().numpy(), z2r.cpu().numpy(), q.cpu().numpy(),
                             np.ones((B, V), np.uint8), *c, relu_z1=relu, up=up)
            bound = (3 * T + 2) * U24 * r[4]
            assert np.all(np.abs(gq.cpu().numpy() - r[2]) <= bound), (up, relu)
            assert np.all(np.abs(wq.cpu().numpy() - r[2]) <= bound)          # (the existing kernel sits inside the same bound)


@pytest.mark.parametrize("B,V,T", CASES, ids=IDS)
def test_random_masks_against_the_restatement(B, V, T):
    from electrocardio_panorama_amd import ops
    z1, z2r, q = _leads(B, V, T, 3)
    mask = _mask(B, V, 4)
    n = mask.sum(1)
    assert n[0] == 1 and n.min() >= 1
    c = (V - 1, V + 4)                                        # the second draw is >= n_b in every sample, the first in sample 0 (V > 1)
    latent, D, pk = ops.lead_mask_mix_fwd(g(z1), g(z2r), g(mask), g(q), c, picks=True)
    want_pk = ref.picks(mask, *c)
    assert np.array_equal(pk.cpu().numpy(), want_pk)
    l64, _, A = ref.forward(z1, z2r, mask, None, *c)
    err = np.abs(latent.cpu().numpy().astype(np.float64) - l64)
    assert np.all(err <= n[:, None, None] * U24 * A), float((err / np.maximum(n[:, None, None] * U24 * A, 1e-300)).max())
    # D: one rounded multiply of q with the kernel's own latent and the picked rows
    Z1, Z2 = g(z1).view(B, V, 128, T), g(z2r).view(B, V, 128, T)
    idx = torch.arange(B, device=DEV)
    p1, p2 = g(want_pk[:, 0]), g(want_pk[:, 1])
    f = g(q)[:, :, None]
    want_D = torch.cat([f * latent, f * torch.cat([Z1[idx, p1], latent[:, 128:]], 1), f * torch.cat([latent[:, :128], Z2[idx, p2]], 1)], 0)
    assert torch.equal(D, want_D)
    # the latent-only form, a second launch, bool masks and device draws: the same bits
    lat_only, none = ops.lead_mask_mix_fwd(g(z1), g(z2r), g(mask), None)
    assert none is None and torch.equal(lat_only, latent)
    again = ops.lead_mask_mix_fwd(g(z1), g(z2r), g(mask).bool(), g(q), torch.tensor(c, dtype=torch.int32, device=DEV), picks=True)
    assert all(torch.equal(a, b) for a, b in zip(again, (latent, D, pk)))
    # backward (gD at the latent's resolution: the bounds are those of the expressions as written)
    rng = np.random.default_rng(5)
    gD = rng.standard_normal((3 * B, 256, T), dtype=np.float32)
    outs = {}
    for relu in (False, True):
        gz1, gz2r, gq = ops.lead_mask_mix_bwd(g(gD), latent, g(z1), g(z2r), g(q), g(mask), c, relu_z1=relu)
        r1, r2, rq, Mz, Mq = ref.backward(gD, latent.cpu().numpy(), z1, z2r, q, mask, *c, relu_z1=relu)
        for got, want, half in ((gz1, r1, Mz[:, :128]), (gz2r, r2, Mz[:, 128:])):
            got = got.cpu().numpy().reshape(B, V, 128, T)
            assert not got[mask == 0].any()                   # absent rows: exact zeros
            e = np.abs(got.astype(np.float64) - want.reshape(B, V, 128, T))
            assert np.all(e <= 4 * U24 * half[:, None]), relu
        assert np.all(np.abs(gq.cpu().numpy() - rq) <= (3 * T + 2) * U24 * Mq)
        outs[relu] = (gz1, gz2r, gq)
        again = ops.lead_mask_mix_bwd(g(gD), latent, g(z1), g(z2r), g(q), g(mask), c, relu_z1=relu)
        assert all(torch.equal(a, b) for a, b in zip(again, outs[relu]))
    # through the upsampling adjoint: the bits of the two-pass form (nef_upsample2_bwd, then the entry at the latent's resolution)
    gU = g(rng.standard_normal((3 * B, 256, 2 * T), dtype=np.float32))
    a = ops.lead_mask_mix_bwd(gU, latent, g(z1), g(z2r), g(q), g(mask), c, up=True, relu_z1=True)
    b = ops.lead_mask_mix_bwd(ops.upsample2_bwd(gU), latent, g(z1), g(z2r), g(q), g(mask), c, relu_z1=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    r = ref.backward(gU.cpu().numpy(), latent.cpu().numpy(), z1, z2r, q, mask, *c, relu_z1=True, up=True)
    assert np.all(np.abs(a[2].cpu().numpy() - r[2]) <= (3 * T + 2) * U24 * r[4])
    # absent leads are never read: NaNs there, and other finite values there, leave every output bit
    if (mask == 0).any():
        for value in (np.nan, 1e30):
            f1, f2 = g(_fill_absent(z1, mask, value)), g(_fill_absent(z2r, mask, value))
            got = ops.lead_mask_mix_fwd(f1, f2, g(mask), g(q), c, picks=True)
            assert all(torch.equal(x, y) for x, y in zip(got, (latent, D, pk))) and bool(torch.isfinite(got[1]).all())
            gb = ops.lead_mask_mix_bwd(g(gD), latent, f1, f2, g(q), g(mask), c, relu_z1=True)
            assert all(torch.equal(x, y) for x, y in zip(gb, outs[True])) and all(bool(torch.isfinite(x).all()) for x in gb)
    else:
        assert V == 1


@pytest.mark.parametrize("T", [3, 65, 130])
def test_a_sample_without_a_present_lead(T):
    from electrocardio_panorama_amd import ops
    B, V = 3, 3
    z1, z2r, q = _leads(B, V, T, 6)
    mask = np.array([[1, 0, 1], [0, 0, 0], [0, 1, 0]], np.uint8)
    z1[1], z2r[1] = np.nan, np.nan                            # nothing of that sample is read
    c = (1, 2)
    latent, D, pk = ops.lead_mask_mix_fwd(g(z1), g(z2r), g(mask), g(q), c, picks=True)
    assert pk.tolist() == [[2, 0], [-1, -1], [1, 1]]
    Dv = D.view(3, B, 256, T)
    assert not latent[1].any() and not Dv[:, 1].any()
    assert not torch.signbit(latent[1]).any() and not torch.signbit(Dv[:, 1]).any()        # +0.0
    assert bool(torch.isfinite(latent).all()) and bool(torch.isfinite(D).all())
    l64 = ref.forward(z1, z2r, mask, None, *c)[0]
    assert np.abs(latent.cpu().numpy() - l64).max() < 1e-5
    rng = np.random.default_rng(7)
    for up in (False, True):
        gD = rng.standard_normal((3 * B, 256, 2 * T if up else T), dtype=np.float32)
        gD.reshape(3, B, 256, -1)[:, 1] = np.nan
        gz1, gz2r, gq = ops.lead_mask_mix_bwd(g(gD), latent, g(z1), g(z2r), g(q), g(mask), c, up=up, relu_z1=True)
        assert not gz1[1].any() and not gz2r[1].any() and not gq[1].any()
        assert all(bool(torch.isfinite(t).all()) for t in (gz1, gz2r, gq)) and bool(gq[0].any()) and bool(gz1[2].any())


def test_unaligned_tensors_take_the_element_path_with_the_same_bits():
    """Views 4 bytes behind a 16-byte boundary: the entry falls back to 4-byte accesses; same expressions, same bits."""
    from electrocardio_panorama_amd import ops
    B, V, T = 2, 3, 37
    z1, z2r, q = _leads(B, V, T, 8)
    mask = _mask(B, V, 9)
    c = (2, 7)

    def off(a):
        buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
        v = buf[1:].view(a.shape)
        v.copy_(g(a))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    want = ops.lead_mask_mix_fwd(g(z1), g(z2r), g(mask), g(q), c)
    got = ops.lead_mask_mix_fwd(off(z1), off(z2r), g(mask), g(q), c)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    gD = np.random.default_rng(10).standard_normal((3 * B, 256, T), dtype=np.float32)
    wb = ops.lead_mask_mix_bwd(g(gD), want[0], g(z1), g(z2r), g(q), g(mask), c, relu_z1=True)
    gb = ops.lead_mask_mix_bwd(off(gD), off(want[0].cpu().numpy()), off(z1), off(z2r), g(q), g(mask), c, relu_z1=True)
    assert torch.equal(gb[0], wb[0]) and torch.equal(gb[1], wb[1])
    r = ref.backward(gD, want[0].cpu().numpy(), z1, z2r, q, mask, *c, relu_z1=True)
    for gq in (gb[2], wb[2]):                                 # (the lanes take other positions: the same terms in another order)
        assert np.all(np.abs(gq.cpu().numpy() - r[2]) <= (3 * T + 2) * U24 * r[4])


# ------------------------------------------------------------------------------------------------ 2. nef_augment_mask
@pytest.mark.parametrize("B,V", [(67, 3), (5, 12), (300, 1)])
def test_augment_mask_is_exact(B, V):
    from electrocardio_panorama_amd import augment, ops
    from test_augment_gpu import make_cfg
    L = 8
    x = g(np.random.default_rng(B).random((B, V, L), dtype=np.float32) + 0.5)          # no zero rows
    rois = torch.zeros(B, 7, 2, dtype=torch.int64, device=DEV)
    for p in (0.3, 0.9):
        aug = augment.from_cfg(make_cfg(V, data=dict(aug_lead_drop=p)))
        for seed, word in ((11, None), (1000, 234), ((1 << 63) + 5, 77)):
            sd = None if word is None else torch.tensor([word], dtype=torch.int64, device=DEV)
            mask = ops.augment_mask(B, V, p, seed=seed, seed_dev=sd, device=DEV)
            assert mask.dtype == torch.uint8 and tuple(mask.shape) == (B, V)
            want = ref.drop_mask((seed + (word or 0)) & ((1 << 64) - 1), B, V, p)
            assert np.array_equal(mask.cpu().numpy(), want)
            y = ops.augment(x, rois, aug, seed=seed, seed_dev=sd)
            assert torch.equal(mask == 0, (y == 0).all(dim=2))
            assert bool(mask.any(dim=1).all())
            out = torch.full((B, V), 9, dtype=torch.uint8, device=DEV)
            assert ops.augment_mask(B, V, p, seed=seed, seed_dev=sd, out=out) is out and torch.equal(out, mask)
    if V == 3:
        m9 = ops.augment_mask(B, V, 0.9, seed=11, device=DEV)
        assert int((m9.sum(1) == 1).sum()) > B // 2                                    # the all-dropped fallback is in the sample
    assert bool(ops.augment_mask(B, V, 0.0, seed=3, device=DEV).all())


# ------------------------------------------------------------------------------------------------ 3. the model
class Cfg(dict):
    __getattr__ = dict.__getitem__


def make_cfg(V, lr=0.1, data=None, model=None, **solver):
    cfg = Cfg(MODEL=Cfg(model="model_nefnet", theta_L=1, loss="v1", resume=""),
              DATA=Cfg(lead_num=V, noise=False, synthetic=True),
              SOLVER=Cfg(optim="sgd", lr=lr, scheduler="MultiStep", lr_step=[50, 100], reg_loss="l1_loss",
                         loss_using=[1, 2, 3], loss_factor=[0.5, 0.5, 1], epochs=1),
              output_dir="/tmp/nef_test", desc="debug", seed=7)
    cfg.MODEL.update(model or {})
    cfg.DATA.update(data or {})
    cfg.SOLVER.update(solver)
    return cfg


ON = dict(data=dict(aug_lead_drop=0.4), model=dict(lead_mask=True))
SHARED = ("decoder.", "mlp1.", "mlp2.", "w_feature_extractor.")
KEEP = [0, 2]                                                 # the mask {0, 2} of the three-lead model


def batch_t(B, V, L, seed, Q=4):
    from electrocardio_panorama_amd import synth
    b = synth.make_batch(B, V, L, seed=seed, Q=Q)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in b.items()}


def _blocks(t, V, keep):
    n = t.shape[0] // V
    return torch.cat([t[v * n:(v + 1) * n] for v in keep], 0)


def _state3():
    from oracle import hashweights as hw
    return {**hw.hashed_params(3), **hw.hashed_buffers()}


def _models(kind):
    """(the three-lead model, the two-lead sub-model of its leads 0 and 2) on the hashed weights, dropout off."""
    from electrocardio_panorama_amd.network import build_model
    from electrocardio_panorama_amd.network.model_nefnet import Model_nefnet2
    if kind == "nefnet2":
        from oracle import hashweights as hw
        full, sub = Model_nefnet2(1, 3).float(), Model_nefnet2(1, 2).float()
        for m in (full, sub):                                 # one shared single-lead encoder: the same state dict
            m.load_state_dict({**hw.hashed_params2(), **hw.hashed_buffers()})
    else:
        full, sub = build_model(make_cfg(3)).float(), build_model(make_cfg(2)).float()
        sd = _state3()
        full.load_state_dict(sd)
        sub.load_state_dict({k: (v if k.startswith(SHARED) or v.dim() == 0 else _blocks(v, 3, KEEP)) for k, v in sd.items()})
    for m in (full, sub):
        m.to(DEV)
        m.dropout_p = 0.0
    return full, sub


def _paired_seeds():
    """random.seed values whose two Standin draws correspond: the three-lead model draws (c1, c2) from 0..2 and picks P[c mod 2] of
    P = [0, 2]; the sub-model has to draw (c1 mod 2, c2 mod 2) from 0..1.  The first pair with a draw >= n_b = 2 and two different picks."""
    for s3 in range(200):
        random.seed(s3)
        a = (random.randint(0, 2), random.randint(0, 2))
        if 2 not in a or a[0] % 2 == a[1] % 2:
            continue
        for s2 in range(200):
            random.seed(s2)
            if (random.randint(0, 1), random.randint(0, 1)) == (a[0] % 2, a[1] % 2):
                return s3, s2
    raise AssertionError("no pair of seeds qualifies")


def _sub_batch(b):
    return dict(b, data=b["data"][:, KEEP].contiguous(), input_theta=b["input_theta"][:, KEEP].contiguous())


def _step(m, b, seed, cfg, **kw):
    from electrocardio_panorama_amd.network import build_loss
    m.train()
    m.zero_grad()
    random.seed(seed)
    o = m(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train", **kw)
    build_loss(cfg)(o[0], o[1], o[2], b["target_view"].unsqueeze(1), cfg)[0].backward()
    torch.cuda.synchronize()
    return [t.detach() for t in o], {n: p.grad for n, p in m.named_parameters()}


class _G:
    def __init__(self, grad):
        self.grad = grad


def _parity(got, want, B, L, factor):
    dead = [n for n, v in want.items() if v is None]
    return assert_grad_parity(got, {n: _G(v) for n, v in want.items()}, dead=dead, flat_tol=factor * FLAT_TOL, tensor_tol=factor * TENSOR_TOL,
                              n_terms=3.0 * B * L)


@pytest.mark.parametrize("kind", ["nefnet", "nefnet2"])
def test_masked_step_is_the_step_of_the_sub_model(kind):
    """B = 4, L = 512, V = 3, dropout off, the mask {0, 2} on every sample: outputs and gradients of the masked train step against the
    unmasked step of the two-lead sub-model on x[:, [0, 2]] at corresponding Standin draws.  Both sides are device paths, each within the
    single bars of its oracle, so the bars are twice tests/test_views_gpu.py's: outputs 2 FWD_TOL, flat gradient 2 FLAT_TOL, per tensor
    2 TENSOR_TOL.  Measured on MI355X, worst ratios to those doubled bars: Model_nefnet outputs 1.4e-7 (0.007 of the bar), flat gradient
    6.6e-7 (0.003), worst tensor W_encoder.layer1.0.conv1.weight 1.5e-6 (0.0008); Model_nefnet2 outputs 1.3e-7 (0.006), flat 8.9e-7
    (0.004), worst tensor W_encoder.layer1.0.conv1.weight 2.1e-6 (0.001).  Model_nefnet additionally has exact zeros in every parameter
    block of the absent lead."""
    B, L = 4, 512
    full, sub = _models(kind)
    b = batch_t(B, 3, L, 31)
    s3, s2 = _paired_seeds()
    mask = torch.tensor([[1, 0, 1]] * B, dtype=torch.bool, device=DEV)
    cfg3, cfg2 = make_cfg(3), make_cfg(2)
    o3, g3 = _step(full, b, s3, cfg3, lead_mask=mask)
    o2, g2 = _step(sub, _sub_batch(b), s2, cfg2)
    worst_o = max(rel(a, w) for a, w in zip(o3, o2))
    assert worst_o < 2 * FWD_TOL, worst_o
    if kind == "nefnet":
        mapped = {}
        for n, v in g3.items():
            if v is None or n.startswith(SHARED):
                mapped[n] = v
                continue
            k = v.shape[0] // 3
            assert not v[k:2 * k].any(), n                    # the absent lead's parameter block: exact zeros
            assert bool(v[:k].any()) and bool(v[2 * k:].any()), n
            mapped[n] = _blocks(v, 3, KEEP)
    else:
        mapped = g3
    flat, worst = _parity(mapped, g2, B, L, 2)
    print(f"masked {kind} step vs the two-lead sub-model: outputs {worst_o:.2e} (bar {2 * FWD_TOL:g}), flat gradient {flat:.2e} "
          f"(bar {2 * FLAT_TOL:g}), worst tensor {worst[1]} {worst[0]:.2e} (bar {2 * TENSOR_TOL:g})")
    # ... and it is not the unmasked three-lead step
    full2, _ = _models(kind)
    o3u, _ = _step(full2, b, s3, cfg3)
    assert rel(o3u[0], o3[0]) > 10 * FWD_TOL


def _decisions(m, o, b):
    """Every ReLU and L1-sign decision of the step just run (tests/decisions.py), for a count of the ones two routes took differently."""
    from decisions import gpu_decisions
    dm = gpu_decisions(m, o, b["target_view"].unsqueeze(1))
    m.last_saved = None
    return {k: v for k, v in dm.items() if not callable(v)}


@pytest.mark.parametrize("B,L", [(4, 512), (2, 5000)], ids=["L512", "L5000"])
def test_all_ones_mask_against_the_unmasked_step(B, L):
    """The three-pass masked head with every lead present against the step as it runs today (shared first conv, fused un-pooling) -- the
    single bars.  L = 5000 is the three-pass head at the flagship's T = 1250.
    The two routes round differently (outputs 1.5e-7 apart), so a ReLU whose argument sits at the switching point can fall either way,
    and one such position moves the gradient by its whole contribution: the batch is screened to be tie-free between the routes, as the
    tie-free golden fixtures are, and the test asserts that it is.  Measured on MI355X, synth.make_batch seeds 31 / 33..36, Standin seed 3:
      B=4 L=512: seed 31 no decision differs, flat gradient 7.1e-7, worst tensor 1.6e-6; seed 33 one flipped decision
        (pass1.decoder.3.double_conv.1), flat 5.2e-4, worst 1.0e-3 -- and 7.7e-7 / 1.9e-6 on the same batch at another Standin draw;
      B=2 L=5000: seeds 31, 34, 36 none, flat 3.8e-7 .. 4.2e-7, worst 5.9e-7 .. 9.5e-7; seed 33 two flips, flat 2.3e-4; seed 35 three, 8.6e-5."""
    cfg = make_cfg(3)
    b = batch_t(B, 3, L, 31)
    ma, _ = _models("nefnet")
    mb, _ = _models("nefnet")
    ma.keep_saved = mb.keep_saved = True
    o1, g1 = _step(ma, b, 3, cfg, lead_mask=torch.ones(B, 3, dtype=torch.uint8, device=DEV))
    d1 = _decisions(ma, o1, b)
    o0, g0 = _step(mb, b, 3, cfg)
    d0 = _decisions(mb, o0, b)
    flips = {k: int((d1[k] != d0[k]).sum()) for k in d1 if not torch.equal(d1[k], d0[k])}
    assert d1.keys() == d0.keys() and len(d1) > 20 and not flips, flips          # the precondition: a tie-free batch
    worst_o = max(rel(a, w) for a, w in zip(o1, o0))
    assert worst_o < FWD_TOL, worst_o
    flat, worst = _parity(g1, g0, B, L, 1)
    print(f"all-ones mask vs the unmasked step (B={B}, L={L}): outputs {worst_o:.2e}, flat gradient {flat:.2e}, worst tensor {worst[1]} {worst[0]:.2e}")


PANO_ATOL = 1e-5            # tests/test_recording_gpu.py's panorama test: views (sigmoid outputs in [0, 1]) within 1e-5


@pytest.mark.parametrize("kind", ["nefnet", "nefnet2"])
def test_masked_inference_is_the_sub_models(kind):
    """panorama, locate(levels=0) and gen_ecg of the three-lead model with the mask {0, 2} against the same calls on the two-lead
    sub-model, all at PANO_ATOL = 1e-5: the views, locate's level-0 scores and score0; the located theta and index are the sub-model's.
    Lead 1 of the batch is then zeroed, as a user without that electrode would feed it: the masked panorama stays at the sub-model's, the
    unmasked one does not.  gen_ecg takes Model_nefnet's per-lead pair; Model_nefnet2's phase 'gen' returns the two means with the mask
    already applied, so its gen_ecg takes none (a [B, 3] mask does not fit the one-lead pair and is rejected by shape).
    Measured on MI355X, both model classes: views, level-0 scores (values up to 0.19 / 0.23) and score0 differ by 0.0 -- the masked
    latent has the sub-model's bits; with lead 1 zeroed the masked views still differ by 0.0, the unmasked ones by 3.5e-3 (Model_nefnet)
    and 1.4e-2 (Model_nefnet2)."""
    from electrocardio_panorama_amd import locate
    B, L = 2, 512
    full, sub = _models(kind)
    full.eval(), sub.eval()
    b = batch_t(B, 3, L, 35, Q=6)
    bs = _sub_batch(b)
    mask = torch.tensor([[1, 0, 1]] * B, dtype=torch.uint8, device=DEV)
    q = b["rest_theta"]
    want = sub.panorama(bs["data"], bs["input_theta"], bs["rois"], q)
    got = full.panorama(b["data"], b["input_theta"], b["rois"], q, lead_mask=mask)
    d_pano = float((got - want).abs().max())
    assert d_pano <= PANO_ATOL, d_pano
    # the recording lacks electrode 1 and is fed zeros there: masked, the sub-model's views; unmasked, the dead lead dilutes them
    x0 = b["data"].clone()
    x0[:, 1] = 0
    got0 = full.panorama(x0, b["input_theta"], b["rois"], q, lead_mask=mask)
    plain0 = full.panorama(x0, b["input_theta"], b["rois"], q)
    d_zero, d_plain = float((got0 - want).abs().max()), float((plain0 - want).abs().max())
    assert d_zero <= PANO_ATOL, d_zero
    assert d_plain > 10 * PANO_ATOL, d_plain
    grid = locate.Grid(3, 4, -4 * np.pi, 6 * np.pi, -6 * np.pi, 6 * np.pi)
    obs = b["rest_view"][:, :2].contiguous()
    r3 = full.locate(b["data"], b["input_theta"], b["rois"], obs, grid=grid, score="mse", levels=0, return_scores=True, lead_mask=mask)
    r2 = sub.locate(bs["data"], bs["input_theta"], bs["rois"], obs, grid=grid, score="mse", levels=0, return_scores=True)
    d_scores, d_score0 = float((r3.scores - r2.scores).abs().max()), float((r3.score0 - r2.score0).abs().max())
    print(f"{kind}: masked panorama vs the sub-model's {d_pano:.2e}; lead 1 zeroed: masked {d_zero:.2e}, unmasked {d_plain:.2e}; "
          f"locate level-0 scores {d_scores:.2e}, score0 {d_score0:.2e}, scores up to {float(r2.scores.abs().max()):.2e}")
    assert d_scores <= PANO_ATOL and d_score0 <= PANO_ATOL, (d_scores, d_score0)
    assert torch.equal(r3.index, r2.index) and torch.equal(r3.theta, r2.theta) and torch.equal(r3.theta0, r2.theta0)
    if kind == "nefnet":                                      # gen_ecg on phase 'gen's per-lead pair (Model_nefnet's form)
        z1, z2 = full(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="gen", lead_mask=mask)
        z1s, z2s = sub(bs["data"], bs["input_theta"], bs["target_theta"], bs["rois"], phase="gen")
        ga = full.gen_ecg(z1, z2, q, b["rois"], lead_mask=mask)
        gs = sub.gen_ecg(z1s, z2s, q, bs["rois"])
        assert torch.allclose(ga, gs, rtol=0, atol=PANO_ATOL) and torch.allclose(ga, got, rtol=0, atol=PANO_ATOL)
    else:                                                     # the two means carry the mask already; the one-lead pair takes no [B, 3] mask
        z1m, z2m = full(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="gen", lead_mask=mask)
        z1s, z2s = sub(bs["data"], bs["input_theta"], bs["target_theta"], bs["rois"], phase="gen")
        assert z1m.shape == (B, 128, L // 4) and torch.allclose(z1m, z1s, rtol=0, atol=PANO_ATOL) and torch.allclose(z2m, z2s, rtol=0, atol=PANO_ATOL)
        with pytest.raises(ValueError, match="lead_mask"):
            full.gen_ecg(z1m, z2m, q, b["rois"], lead_mask=mask)
    with pytest.raises(ValueError, match="lead_mask"):
        full.panorama(b["data"], b["input_theta"], b["rois"], q, lead_mask=mask[:1])
    assert not full.training


@pytest.mark.parametrize("kind", ["nefnet", "nefnet2"])
def test_engine_backward_takes_the_forwards_mask_or_none(kind):
    """engine.backward / backward2(lead_mask=): the mask travels in the saved state; one passed again must be the forward's tensor (a view
    of it counts, a copy with the same content does not -- the check reads nothing on the host) and gives the gradients of passing none."""
    from electrocardio_panorama_amd import ops
    B, L = 2, 512
    full, _ = _models(kind)
    b = batch_t(B, 3, L, 37)
    mask = torch.tensor([[1, 0, 1], [0, 1, 1]], dtype=torch.bool, device=DEV)
    full.train()
    full.keep_saved = True

    def fwd():
        random.seed(5)
        full(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train", lead_mask=mask)
        sv, full.last_saved = full.last_saved, None
        return sv

    P = {n: p.detach() for n, p in full.named_parameters()}
    gs = tuple(torch.randn(B, 1, L, generator=torch.Generator().manual_seed(i)).to(DEV) for i in range(3))
    bwd = full._ENGINE[1]
    with ops.amax_scope((full._nef_scope, True)):
        sv = fwd()
        with pytest.raises(ValueError, match="not the mask the forward ran with"):
            bwd(P, sv, gs, lead_mask=mask.clone())
        with pytest.raises(ValueError, match="not the mask the forward ran with"):
            bwd(P, sv, gs, lead_mask=torch.ones_like(mask))
        with pytest.raises(TypeError, match="bool or uint8"):
            bwd(P, sv, gs, lead_mask=mask.float())
        g_same = bwd(P, sv, gs, lead_mask=mask.view(torch.uint8))
        g_none = bwd(P, fwd(), gs)
    torch.cuda.synchronize()
    assert g_same.keys() == g_none.keys() and len(g_same) > 40
    for n in g_same:      # (two forwards of one model; the conv biases in front of a BatchNorm have an analytically zero gradient)
        if g_same[n] is None or n.endswith(("double_conv.0.bias", "double_conv.3.bias")):
            assert (g_same[n] is None) == (g_none[n] is None), n
            continue
        assert rel(g_same[n], g_none[n]) < TENSOR_TOL, n
    # ... and a state saved without a mask takes none
    full(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
    with ops.amax_scope((full._nef_scope, True)), pytest.raises(ValueError, match="not the mask the forward ran with"):
        bwd(P, full.last_saved, gs, lead_mask=mask)


def test_the_model_derives_its_mask_from_the_dropped_leads(monkeypatch):
    from electrocardio_panorama_amd import augment, ops
    V, B, L = 3, 4, 512
    b = batch_t(B, V, L, 36)
    cfg = make_cfg(V, **ON)
    m, _ = _models("nefnet")
    m.augment, m.lead_mask_from_aug, m.keep_saved = augment.from_cfg(cfg), True, True
    torch.manual_seed(99)
    m._drop_calls = 0
    o, _ = _step(m, b, 4, cfg)
    step_seed = (torch.initial_seed() + 1) & 0x7FFFFFFFFFFF
    fed = ops.augment(b["data"], b["rois"], m.augment, seed=augment.train_seed(step_seed))
    want = (fed != 0).any(dim=2).to(torch.uint8)
    assert torch.equal(m.last_saved["x"], fed) and torch.equal(m.last_saved["mask"], want) and bool((want == 0).any())
    with pytest.raises(ValueError, match="explicit lead_mask"):
        m(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train", lead_mask=want)
    m.eval()                                                  # no corruption, no derived mask; an explicit one is the caller's business
    m(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
    assert m.last_saved["mask"] is None
    m(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train", lead_mask=want)
    assert torch.equal(m.last_saved["mask"], want)


# ------------------------------------------------------------------------------------------------ 4. the step
def _batches(n, B, V, L, seed0, n_rest=5):
    from electrocardio_panorama_amd import synth
    return [dict(synth.make_batch(B, V, L, seed=seed0 + s, Q=n_rest)) for s in range(n)]


def _solver_from(cfg):
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from oracle import hashweights as hw
    torch.manual_seed(1234)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.load_state_dict({**hw.hashed_params(cfg.DATA.lead_num), **hw.hashed_buffers()})
    sol.model.dropout_p = 0.0
    return cfg, sol, get_optimizer(cfg, sol.model.parameters())


def _solver(V, optim, graph, accum=1, **keys):
    cfg = make_cfg(V, lr={"sgd": 0.1, "adam": 1e-3}[optim], optim=optim, graph=bool(graph), **ON, **keys)
    if accum > 1:
        cfg.SOLVER["accum_steps"] = accum
    return _solver_from(cfg)


_SLOTS = {"sgd": ("buf",), "adam": ("m", "v", "step")}


def _state(sol, opt, optim):
    fl = opt._flat[0]
    return [fl["p"].clone()] + [fl[k].clone() for k in _SLOTS[optim]] + [v.clone() for k, v in sol.model.named_buffers()]


def _three_steps(sol, opt, batches):
    """Two epochs (two batches, one batch) with a MultiStepLR milestone crossed between them: the loss rows of the three steps."""
    from torch.optim.lr_scheduler import MultiStepLR
    sched = MultiStepLR(opt, [1], gamma=0.1)
    rows = []
    for i, part in enumerate((batches[:2], batches[2:])):
        random.seed(100 + i)
        rows += sol.run_one_epoch(part, "train", opt, collect_views=False)[0]
        sched.step()
    return np.array(rows)


@pytest.mark.parametrize("optim,accum,views", [("sgd", 1, 1), ("adam", 1, 1), ("sgd", 2, 1), ("sgd", 1, 2)],
                         ids=["sgd", "adam", "sgd_accum2", "sgd_views2"])
def test_lead_mask_graphed_equals_eager(optim, accum, views, monkeypatch):
    """Three steps at (B=2, V=3, L=512) with MODEL.lead_mask and aug_lead_drop 0.4 across an LR milestone: the replayed step equals the
    eager one bit for bit -- parameters, optimiser state, BatchNorm buffers, loss rows; the static mask of the last replay is the eager
    step's."""
    from electrocardio_panorama_amd import ops
    V, B, L = 3, 2, 512
    batches = _batches(3, B, V, L, 40)
    keys = dict(train_views=views) if views > 1 else {}
    out, masks = {}, []
    real = ops.augment_mask
    for graph in (False, True):
        cfg, sol, opt = _solver(V, optim, graph, accum=accum, **keys)
        assert sol.lead_mask is True and sol.model.lead_mask_from_aug is True
        if not graph:
            monkeypatch.setattr(ops, "augment_mask", lambda *a, **k: (lambda y: (masks.append(y.clone()), y)[1])(real(*a, **k)))
        else:
            monkeypatch.setattr(ops, "augment_mask", real)
        rows = _three_steps(sol, opt, batches)
        assert rows.shape == (3, 4) and np.isfinite(rows).all()
        st = getattr(sol, "_graph_stepper", None)
        assert (st is not None) == graph
        if graph:
            assert st.calls == 1 and len(st.slots) == 1 and st.lead_mask_on and st.lead_mask.dtype == torch.uint8 and tuple(st.lead_mask.shape) == (B, V)
            assert torch.equal(st.lead_mask, masks[-1])
        out[graph] = (_state(sol, opt, optim), rows)
    assert len(masks) == 3 and any(bool((m == 0).any()) for m in masks)          # a lead was dropped somewhere in the three steps
    for a, b in zip(out[False][0], out[True][0]):
        assert torch.equal(a, b)
    assert np.array_equal(out[False][1], out[True][1])


def test_key_on_is_another_step_and_key_off_is_todays():
    """Same seeds, same dropped leads: with MODEL.lead_mask the losses differ from the key off (the dead lead no longer enters the mean);
    with the key False the loss rows and parameters are those of a config that has no such key, bit for bit."""
    V, B, L = 3, 2, 512
    batches = _batches(3, B, V, L, 40)
    runs = {}
    models = dict(on=dict(lead_mask=True), off=dict(lead_mask=False), absent={})
    for name, model in models.items():
        cfg, sol, opt = _solver_from(make_cfg(V, graph=True, data=ON["data"], model=model))
        assert ("lead_mask" in cfg.MODEL) == (name != "absent") and sol.lead_mask == (name == "on")
        rows = _three_steps(sol, opt, batches)
        runs[name] = (rows, _state(sol, opt, "sgd"))
        assert (sol._graph_stepper.lead_mask is not None) == (name == "on")
    assert np.array_equal(runs["off"][0], runs["absent"][0])
    for a, b in zip(runs["off"][1], runs["absent"][1]):
        assert torch.equal(a, b)
    assert not np.array_equal(runs["on"][0][:, 0], runs["off"][0][:, 0])
    assert np.abs(runs["on"][0][:, 0] - runs["off"][0][:, 0]).max() > 1e-4


def _loader_solver(graph):
    from electrocardio_panorama_amd.solver import Solver
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    from electrocardio_panorama_amd.train_net import SyntheticLoader
    cfg = make_cfg(3, graph=bool(graph), **ON)
    torch.manual_seed(1234)
    sol = Solver(cfg, use_tensorboardx=False)
    sol.model.dropout_p = 0.0
    return cfg, sol, get_optimizer(cfg, sol.model.parameters()), SyntheticLoader(cfg, batch_size=4, n_batches=2, length=512, seed=cfg.seed)


def _epoch(sol, opt, dl, epoch):
    sol.model.dropout_epoch = epoch
    random.seed(100 + epoch)
    return np.array(sol.run_one_epoch(dl, "train", opt, collect_views=False)[0])


def test_a_resumed_epoch_reproduces_the_uninterrupted_one():
    """B=4, L=512, 2 batches per epoch, replayed masked steps: epoch 1 run by a fresh Solver from epoch 0's state equals the uninterrupted
    epoch 1 bit for bit -- the mask is a function of (seed, epoch, batch index, rank), not of any state."""
    cfg, sol_g, opt_g, dl = _loader_solver(True)
    rows_0 = _epoch(sol_g, opt_g, dl, 0)
    model_sd = {k: v.detach().clone() for k, v in sol_g.model.state_dict().items()}
    h2_blob = sol_g.model.h2_state()
    opt_sd = opt_g.state_dict()
    opt_sd = {"state": {k: {kk: (vv.clone() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in opt_sd["state"].items()},
              "param_groups": opt_sd["param_groups"]}
    rows_1 = _epoch(sol_g, opt_g, dl, 1)
    assert not np.array_equal(rows_0, rows_1)
    cfg, sol_r, opt_r, dl = _loader_solver(True)
    sol_r.model.load_state_dict(model_sd)
    sol_r.model.load_h2_state(h2_blob)
    opt_r.load_state_dict(opt_sd)
    rows_r = _epoch(sol_r, opt_r, dl, 1)
    assert np.array_equal(rows_1, rows_r)
    for (n, a), (_, b) in zip(sol_g.model.state_dict().items(), sol_r.model.state_dict().items()):
        assert torch.equal(a, b), n


def test_aug_eval_hands_the_model_the_mask_of_its_own_seed(monkeypatch):
    """The DATA.aug_eval pass of the test phase: the model gets the mask of the leads that pass's fixed seed dropped; the clean test
    phase passes none and keeps its numbers."""
    from electrocardio_panorama_amd import augment, ops, synth
    from electrocardio_panorama_amd.solver import Solver
    V, B, L = 3, 4, 512
    test = [dict(synth.make_batch(B, V, L, seed=70 + i, Q=6)) for i in range(2)]
    seen = []

    def run(on):
        cfg = make_cfg(V, data=dict(aug_lead_drop=0.4, aug_eval=True), model=dict(lead_mask=True) if on else {})
        torch.manual_seed(1234)
        sol = Solver(cfg, use_tensorboardx=False)
        real = sol.model.forward

        def spy(*a, **k):
            seen.append((on, k.get("lead_mask"), a[0].clone()))
            return real(*a, **k)

        monkeypatch.setattr(sol.model, "forward", spy)
        with torch.no_grad():
            clean = sol.run_one_epoch(test, phase="test", collect_views=False)[4]
            aug = sol.run_one_epoch(test, phase="test", collect_views=False, aug_eval=True)[4]
        return np.array(clean), np.array(aug)

    clean_on, aug_on = run(True)
    clean_off, aug_off = run(False)
    assert np.array_equal(clean_on, clean_off)                                   # the clean numbers keep their bits
    assert not np.array_equal(aug_on, aug_off)
    on = [s for s in seen if s[0]]
    assert len(on) == 4 and all(m is None for _, m, _ in on[:2])                 # the clean pass: no mask
    for i, (_, m, x) in enumerate(on[2:]):
        want = ops.augment_mask(B, V, 0.4, seed=augment.eval_seed(7, i, 0), device=DEV)
        assert torch.equal(m, want) and torch.equal(m == 0, (x == 0).all(dim=2))
    assert any(bool((m == 0).any()) for _, m, _ in on[2:])
    assert all(m is None for flag, m, _ in seen if not flag)
