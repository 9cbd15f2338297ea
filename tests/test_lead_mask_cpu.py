"""MODEL.lead_mask without a GPU: the numpy restatement the GPU tests compare against (tests/lead_mask_ref.py) held to literal loops
and to torch autograd, the drop mask held to augment_ref's output, every wrapper's argument checks (in front of the library), the
config's rejection, and "off is off"."""
import itertools

import numpy as np
import pytest
import torch

import augment_ref
import lead_mask_ref as ref


def _cfg(lead_mask=None, **data):
    from electrocardio_panorama_amd.config.default import get_defaults
    cfg = get_defaults()
    for k, v in data.items():
        cfg.DATA[k] = v
    if lead_mask is not None:
        cfg.MODEL.lead_mask = lead_mask
    return cfg


def _literal(mask_row, c):
    """P_b[c mod n_b] by counting through the row."""
    n = sum(1 for m in mask_row if m)
    if n == 0:
        return -1
    k = c % n
    for v, m in enumerate(mask_row):
        if m:
            if k == 0:
                return v
            k -= 1
    raise AssertionError


def test_picks_and_present_lists_every_small_mask():
    for V in range(1, 5):
        rows = list(itertools.product((0, 1), repeat=V))
        mask = np.array(rows, np.uint8)
        lists = ref.present_lists(mask)
        for row, P in zip(rows, lists):
            assert P == [v for v in range(V) if row[v]] and P == sorted(P)
        for c1, c2 in ((0, 0), (1, 3), (V - 1, V), (7, 2), (11, 5)):
            pk = ref.picks(mask, c1, c2)
            for b, row in enumerate(rows):
                assert tuple(pk[b]) == (_literal(row, c1), _literal(row, c2)), (row, c1, c2)
        # all ones: the draws themselves
        ones = np.ones((1, V), np.uint8)
        for c in range(V):
            assert tuple(ref.picks(ones, c, V - 1 - c)[0]) == (c, V - 1 - c)


def test_picks_random_masks_of_twelve_leads():
    rng = np.random.default_rng(3)
    mask = (rng.random((64, 12)) < 0.5).astype(np.uint8) * rng.integers(1, 255, (64, 12), dtype=np.uint8)      # any non-zero byte is "present"
    mask[0] = 0
    mask[1] = 0
    mask[1, 11] = 200
    for c1, c2 in ((0, 11), (5, 7), (13, 40)):
        pk = ref.picks(mask, c1, c2)
        for b in range(64):
            assert tuple(pk[b]) == (_literal(mask[b], c1), _literal(mask[b], c2))
    assert tuple(ref.picks(mask, 3, 4)[0]) == (-1, -1) and tuple(ref.picks(mask, 3, 4)[1]) == (11, 11)


def _torch_forward(z1, z2r, mask, q, c1, c2):
    """The definition written with torch ops (fp64, differentiable): latent, D."""
    B, V = mask.shape
    T = z1.shape[2]
    Z1, Z2 = z1.view(B, V, 128, T), z2r.view(B, V, 128, T)
    lat, d = [], [[], [], []]
    for b in range(B):
        P = [v for v in range(V) if mask[b, v]]
        if not P:
            zero = torch.zeros(256, T, dtype=z1.dtype)
            lat.append(zero)
            for p in range(3):
                d[p].append(zero)
            continue
        m1 = sum(Z1[b, v] for v in P) / len(P)
        m2 = sum(Z2[b, v] for v in P) / len(P)
        latent = torch.cat([m1, m2], 0)
        f = q[b][:, None]
        lat.append(latent)
        d[0].append(f * latent)
        d[1].append(f * torch.cat([Z1[b, P[c1 % len(P)]], m2], 0))
        d[2].append(f * torch.cat([m1, Z2[b, P[c2 % len(P)]]], 0))
    return torch.stack(lat), torch.cat([torch.stack(p) for p in d], 0)


@pytest.mark.parametrize("mask,c1,c2", [([[1, 0, 1], [0, 1, 0]], 1, 2), ([[1, 1, 1], [1, 1, 1]], 2, 0), ([[0, 0, 0], [1, 1, 0]], 4, 1)],
                         ids=["mixed", "all_ones", "empty_sample"])
def test_restated_backward_against_autograd(mask, c1, c2):
    B, V, T = 2, 3, 5
    g = torch.Generator().manual_seed(11)
    z1 = torch.randn(B, 128 * V, T, generator=g, dtype=torch.float64, requires_grad=True)
    z2r = torch.randn(B, 128 * V, T, generator=g, dtype=torch.float64, requires_grad=True)
    q = torch.randn(B, 256, generator=g, dtype=torch.float64, requires_grad=True)
    gD = torch.randn(3 * B, 256, T, generator=g, dtype=torch.float64)
    mask = np.array(mask, np.uint8)
    latent, D = _torch_forward(z1, z2r, mask, q, c1, c2)
    lat_ref, D_ref, _ = ref.forward(z1.detach().numpy(), z2r.detach().numpy(), mask, q.detach().numpy(), c1, c2)
    assert np.abs(lat_ref - latent.detach().numpy()).max() < 1e-12 and np.abs(D_ref - D.detach().numpy()).max() < 1e-12
    D.backward(gD)
    gz1, gz2r, gq, Mz, Mq = ref.backward(gD.numpy(), lat_ref, z1.detach().numpy(), z2r.detach().numpy(), q.detach().numpy(), mask, c1, c2)
    for got, want in ((gz1, z1.grad), (gz2r, z2r.grad), (gq, q.grad)):
        assert np.abs(got - want.numpy()).max() < 1e-12
    # absent rows are exact zeros; the magnitudes dominate the values
    for b in range(B):
        for v in range(V):
            if not mask[b, v]:
                assert not gz1[b, v * 128:(v + 1) * 128].any() and not gz2r[b, v * 128:(v + 1) * 128].any()
    assert np.all(np.abs(gq) <= Mq + 1e-12)


def test_restated_backward_through_the_upsampling_and_the_relu_mask():
    B, V, T = 2, 3, 5
    g = torch.Generator().manual_seed(12)
    z1 = torch.randn(B, 128 * V, T, generator=g, dtype=torch.float64)
    z2r = torch.randn(B, 128 * V, T, generator=g, dtype=torch.float64)
    q = torch.randn(B, 256, generator=g, dtype=torch.float64)
    gU = torch.randn(3 * B, 256, 2 * T, generator=g, dtype=torch.float64)
    mask = np.array([[1, 0, 1], [1, 1, 1]], np.uint8)
    # the adjoint of torch's own upsampling
    x = torch.zeros(3 * B, 256, T, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.interpolate(x, scale_factor=2, mode="linear", align_corners=False).backward(gU)
    lat = ref.forward(z1.numpy(), z2r.numpy(), mask, None, 0, 0)[0]
    a = ref.backward(gU.numpy(), lat, z1.numpy(), z2r.numpy(), q.numpy(), mask, 1, 2, up=True)
    b = ref.backward(x.grad.numpy(), lat, z1.numpy(), z2r.numpy(), q.numpy(), mask, 1, 2)
    for got, want in zip(a[:3], b[:3]):
        assert np.abs(got - want).max() < 1e-12
    r = ref.backward(x.grad.numpy(), lat, z1.numpy(), z2r.numpy(), q.numpy(), mask, 1, 2, relu_z1=True)
    assert np.array_equal(r[0], np.where(z1.numpy() > 0, b[0], 0.0)) and np.array_equal(r[1], b[1]) and np.array_equal(r[2], b[2])


def test_fp32_order_of_the_mean():
    """The float32 replay is the defined order: it differs from the rounded fp64 mean by at most the bound the GPU test uses."""
    rng = np.random.default_rng(5)
    B, V, T = 3, 12, 7
    z1 = rng.standard_normal((B, 128 * V, T), dtype=np.float32)
    z2r = rng.standard_normal((B, 128 * V, T), dtype=np.float32)
    mask = (rng.random((B, V)) < 0.6).astype(np.uint8)
    mask[0, :] = 0
    mask[0, 4] = 1
    l32, _, _ = ref.forward(z1, z2r, mask, None, 0, 0, dtype=np.float32)
    l64, _, A = ref.forward(z1, z2r, mask, None, 0, 0)
    assert l32.dtype == np.float32
    n = mask.astype(bool).sum(1)[:, None, None]
    assert np.all(np.abs(l32.astype(np.float64) - l64) <= n * ref.U24 * A)
    assert np.array_equal(l32[0], np.concatenate([z1[0, 4 * 128:5 * 128], z2r[0, 4 * 128:5 * 128]], 0))      # n_b = 1: the lead's bits


@pytest.mark.parametrize("p", [0.3, 0.9])
def test_drop_mask_is_the_zero_rows_of_the_restated_augmentation(p):
    B, V, L = 257, 3, 8
    rng = np.random.default_rng(1)
    x = rng.random((B, V, L), dtype=np.float32) + 0.5          # no zero rows
    rois = np.zeros((B, 7, 2), np.int64)
    for seed in (0, 12345, (1 << 62) + 9):
        y, dropped, _ = augment_ref.augment(x, rois, seed, lead_drop=p)
        mask = ref.drop_mask(seed, B, V, p)
        assert mask.dtype == np.uint8 and np.array_equal(mask == 0, (y == 0).all(axis=2)) and np.array_equal(mask == 0, dropped)
        assert mask.any(axis=1).all()                          # every sample keeps a lead
    if p == 0.9:                                               # the all-dropped fallback is in the sample
        _, drew = augment_ref.dropped_rows(12345, B, V, p)
        all3 = drew.all(axis=1)
        assert all3.sum() > 100 and (ref.drop_mask(12345, B, V, p)[all3].sum(axis=1) == 1).all()
    assert ref.drop_mask(7, 4, 3, 0.0).all()


def _untouched(monkeypatch):
    from electrocardio_panorama_amd import _lib

    def touched():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", touched)


def test_mix_wrappers_check_their_arguments_before_the_library(monkeypatch):
    from electrocardio_panorama_amd import ops
    _untouched(monkeypatch)
    B, V, T = 2, 3, 5
    z1, z2r = torch.zeros(B, 128 * V, T), torch.zeros(B, 128 * V, T)
    mask, q = torch.ones(B, V, dtype=torch.uint8), torch.zeros(B, 256)
    gD, lat = torch.zeros(3 * B, 256, T), torch.zeros(B, 256, T)
    for call in (lambda **k: ops.lead_mask_mix_fwd(k.get("z1", z1), k.get("z2r", z2r), k.get("mask", mask), k.get("q", q), k.get("choice", (0, 0))),
                 lambda **k: ops.lead_mask_mix_bwd(k.get("gD", gD), k.get("latent", lat), k.get("z1", z1), k.get("z2r", z2r), k.get("q", q),
                                                   k.get("mask", mask), k.get("choice", (0, 0)), up=k.get("up", False))):
        with pytest.raises(TypeError, match="float32"):
            call(z1=z1.double())
        with pytest.raises(ValueError, match="contiguous"):
            call(z1=z1.transpose(0, 1))
        with pytest.raises(ValueError, match="128 V"):
            call(z1=torch.zeros(B, 100, T), z2r=torch.zeros(B, 100, T))
        with pytest.raises(ValueError, match="V in 1..12"):
            call(z1=torch.zeros(B, 128 * 13, T), z2r=torch.zeros(B, 128 * 13, T))
        with pytest.raises(ValueError, match="z2r"):
            call(z2r=torch.zeros(B, 128 * V, T + 1))
        with pytest.raises(TypeError, match="bool or uint8"):
            call(mask=mask.float())
        with pytest.raises(TypeError, match="bool or uint8"):
            call(mask=None)
        with pytest.raises(ValueError, match=r"is not \[2, 3\]"):
            call(mask=torch.ones(B, V + 1, dtype=torch.bool))
        with pytest.raises(ValueError, match="q"):
            call(q=torch.zeros(B, 128))
        with pytest.raises(TypeError, match="q"):
            call(q=q.double())
        with pytest.raises(TypeError, match="choice"):
            call(choice=(0.5, "a"))
        with pytest.raises(TypeError, match="choice"):
            call(choice=3)
        with pytest.raises(ValueError, match="choice"):
            call(choice=(-1, 0))
        with pytest.raises(ValueError, match="choice"):
            call(choice=torch.zeros(2, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()                                             # CPU tensors, everything else right: still in front of the library
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(mask=mask.bool(), choice=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="gD"):
        ops.lead_mask_mix_bwd(gD, lat, z1, z2r, q, mask, (0, 0), up=True)           # up wants [3B, 256, 2T]
    with pytest.raises(ValueError, match="latent"):
        ops.lead_mask_mix_bwd(gD, lat[:, :128], z1, z2r, q, mask, (0, 0))
    with pytest.raises(TypeError, match="q"):
        ops.lead_mask_mix_bwd(gD, lat, z1, z2r, None, mask, (0, 0))                 # the latent-only form is the forward's
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lead_mask_mix_fwd(z1, z2r, mask, None)


def test_augment_mask_checks_its_arguments_before_the_library(monkeypatch):
    from electrocardio_panorama_amd import ops
    _untouched(monkeypatch)
    for bad in (dict(B=0), dict(V=0), dict(V=13)):
        with pytest.raises(ValueError, match="V in 1..12"):
            ops.augment_mask(**{**dict(B=2, V=3, lead_drop=0.3, device="cpu"), **bad})
    with pytest.raises(TypeError, match="int"):
        ops.augment_mask(2.0, 3, 0.3, device="cpu")
    for p in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="lead_drop"):
            ops.augment_mask(2, 3, p, device="cpu")
    with pytest.raises(ValueError, match="device"):
        ops.augment_mask(2, 3, 0.3)
    with pytest.raises(ValueError, match="out"):
        ops.augment_mask(2, 3, 0.3, out=torch.zeros(2, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="out"):
        ops.augment_mask(2, 3, 0.3, out=torch.zeros(3, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="seed_dev"):
        ops.augment_mask(2, 3, 0.3, device="cpu", seed_dev=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.augment_mask(2, 3, 0.3, out=torch.zeros(2, 3, dtype=torch.uint8), seed_dev=torch.zeros(1, dtype=torch.int64))


def test_model_checks_the_mask_before_anything_runs():
    from electrocardio_panorama_amd.network import build_model
    cfg = _cfg(lead_num=3)
    cfg.MODEL.model = "model_nefnet"
    m = build_model(cfg)
    dev = torch.device("cpu")
    assert m._check_mask(None, 2, 3, dev) is None
    got = m._check_mask(torch.ones(2, 3, dtype=torch.bool), 2, 3, dev)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3)
    with pytest.raises(ValueError, match=r"is not \[2, 3\]"):
        m._check_mask(torch.ones(2, 2, dtype=torch.bool), 2, 3, dev)
    with pytest.raises(TypeError, match="bool or uint8"):
        m._check_mask(torch.ones(2, 3), 2, 3, dev)
    with pytest.raises(TypeError, match="bool or uint8"):
        m._check_mask([[1, 1, 1], [1, 0, 1]], 2, 3, dev)
    with pytest.raises(ValueError, match="is on"):
        m._check_mask(torch.ones(2, 3, dtype=torch.uint8), 2, 3, torch.device("meta"))
    # the keyword is keyword-only on every entry point
    import inspect
    for fn in (m.forward, m.gen_ecg, m.panorama, m.locate):
        assert inspect.signature(fn).parameters["lead_mask"].kind is inspect.Parameter.KEYWORD_ONLY


def test_config_rejects_a_mask_with_nothing_to_mask():
    from electrocardio_panorama_amd import augment
    assert _cfg().MODEL.lead_mask is False and augment.lead_mask_on(_cfg()) is False
    with pytest.raises(ValueError, match="MODEL.lead_mask"):
        augment.from_cfg(_cfg(lead_mask=True))
    with pytest.raises(ValueError, match="MODEL.lead_mask"):
        augment.from_cfg(_cfg(lead_mask=True, aug_noise_std=0.1))        # another corruption on, still no lead dropped
    with pytest.raises(ValueError, match="MODEL.lead_mask"):
        augment.lead_mask_on(_cfg(lead_mask=1))
    a = augment.from_cfg(_cfg(lead_mask=True, aug_lead_drop=0.4))
    assert a.lead_drop == 0.4 and augment.lead_mask_on(_cfg(lead_mask=True, aug_lead_drop=0.4)) is True


def test_off_is_off(monkeypatch):
    """The default config builds no mask anywhere: no attribute set, no buffer, and no call of ops.augment_mask or the masked mix."""
    from electrocardio_panorama_amd import ops
    from electrocardio_panorama_amd.graph import GraphedTrainStep
    from electrocardio_panorama_amd.network import build_model

    def never(*a, **k):
        raise AssertionError("a lead-mask entry was called with the key off")

    for name in ("augment_mask", "lead_mask_mix_fwd", "lead_mask_mix_bwd", "lead_mask_arg"):
        monkeypatch.setattr(ops, name, never)
    for data in (dict(lead_num=3), dict(lead_num=3, aug_lead_drop=0.25)):
        cfg = _cfg(**data)
        cfg.MODEL.model = "model_nefnet"
        m = build_model(cfg)
        assert m.lead_mask_from_aug is False and m._mask_kw(None) == {}
        st = GraphedTrainStep(m, cfg)
        assert st.lead_mask_on is False and st.lead_mask is None
    cfg = _cfg(lead_mask=True, lead_num=3, aug_lead_drop=0.25)
    cfg.MODEL.model = "model_nefnet"
    assert GraphedTrainStep(build_model(cfg), cfg).lead_mask_on is True
