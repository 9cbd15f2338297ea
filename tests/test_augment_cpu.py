"""DATA.aug_* without a GPU: the keys and their rejections (augment.from_cfg), the statistics of the numpy restatement the GPU tests
compare against (tests/augment_ref.py), and ops.augment's argument checks, which sit in front of the library."""
import math

import numpy as np
import pytest
import torch

import augment_ref as ref


def _cfg(**data):
    from electrocardio_panorama_amd.config.default import get_defaults
    cfg = get_defaults()
    for k, v in data.items():
        cfg.DATA[k] = v
    return cfg


def test_defaults_are_off():
    from electrocardio_panorama_amd import augment
    cfg = _cfg()
    for key, want in (("aug_noise_std", 0.0), ("aug_wander_amp", 0.0), ("aug_wander_hz", [0.05, 0.7]), ("aug_hum_amp", 0.0),
                      ("aug_hum_hz", 50.0), ("aug_lead_drop", 0.0), ("sample_rate", 500.0), ("aug_crop", True), ("aug_eval", False)):
        assert cfg.DATA[key] == want, key
    assert augment.from_cfg(cfg) is None
    assert augment.from_cfg(_cfg(aug_eval=True, aug_crop=False)) is None        # no corruption on: nothing to evaluate either


def test_from_cfg_carries_the_keys():
    from electrocardio_panorama_amd import augment
    a = augment.from_cfg(_cfg(aug_noise_std=0.02, aug_wander_amp=0.1, aug_wander_hz=[0.1, 0.5], aug_hum_amp=0.05, aug_hum_hz=60.0,
                              aug_lead_drop=0.25, sample_rate=250.0, aug_crop=False, aug_eval=True))
    assert a == augment.Augment(0.02, 0.1, 0.1, 0.5, 0.05, 60.0, 0.25, 250.0, False, True)
    for only in ("aug_noise_std", "aug_wander_amp", "aug_hum_amp", "aug_lead_drop"):
        a = augment.from_cfg(_cfg(**{only: 0.5}))
        assert a is not None and len(a.active()) == 1 and only in a.describe()


@pytest.mark.parametrize("key,data", [
    ("aug_noise_std", dict(aug_noise_std=-0.1)),
    ("aug_wander_amp", dict(aug_wander_amp=-1.0)),
    ("aug_hum_amp", dict(aug_hum_amp=-1e-3)),
    ("aug_lead_drop", dict(aug_lead_drop=-0.5)),
    ("aug_wander_hz", dict(aug_wander_amp=0.1, aug_wander_hz=[-0.1, 0.7])),
    ("aug_hum_hz", dict(aug_hum_amp=0.1, aug_hum_hz=-50.0)),
    ("aug_lead_drop", dict(aug_lead_drop=1.0)),
    ("aug_lead_drop", dict(aug_lead_drop=1.5)),
    ("aug_wander_hz", dict(aug_wander_amp=0.1, aug_wander_hz=[0.7, 0.05])),
    ("sample_rate", dict(aug_noise_std=0.1, sample_rate=0.0)),
    ("sample_rate", dict(aug_noise_std=0.1, sample_rate=-500.0)),
    ("aug_wander_hz", dict(aug_wander_amp=0.1, aug_wander_hz=[0.05, 250.0])),
    ("aug_wander_hz", dict(aug_wander_amp=0.1, aug_wander_hz=[0.05, 0.7], sample_rate=1.0)),
    ("aug_hum_hz", dict(aug_hum_amp=0.1, aug_hum_hz=250.0)),
    ("aug_hum_hz", dict(aug_hum_amp=0.1, aug_hum_hz=60.0, sample_rate=100.0)),
], ids=["neg_noise", "neg_wander", "neg_hum", "neg_drop", "neg_wander_hz", "neg_hum_hz", "drop_1", "drop_above_1", "lo_above_hi",
        "fs_0", "fs_neg", "wander_at_nyquist", "wander_above_nyquist", "hum_at_nyquist", "hum_above_nyquist"])
def test_rejections_name_the_key(key, data):
    from electrocardio_panorama_amd import augment
    with pytest.raises(ValueError, match="DATA." + key):
        augment.from_cfg(_cfg(**data))


def test_seed_words():
    """The train word is the step's seed plus the site word (what a replayed launch adds up from its host word and seed_dev); the site
    is one behind the last dropout site; an eval seed is no train seed."""
    from electrocardio_panorama_amd import augment, engine
    n = len(engine.DROPOUT_SITES)
    assert augment.site_word() == n * 0x85EBCA6B + 1
    for step in (0, 1, 0x7FFFFFFFFFFF):
        assert augment.train_seed(step) == step + augment.site_word()
    drop_words = {k * 0x85EBCA6B + 1 for k in range(n)}
    assert augment.site_word() not in drop_words
    assert augment.eval_seed(123, 4, 1) == augment.eval_seed(123, 4, 1) != augment.eval_seed(123, 5, 1) != augment.eval_seed(123, 4, 0)
    assert augment.eval_seed(123, 0) >> 48 == 1 and augment.train_seed(0x7FFFFFFFFFFF) >> 48 == 0


def test_restatement_normals():
    N = 1 << 20
    n, r = ref.normals(12345, N)
    assert n.shape == r.shape == (N,)
    assert abs(n.mean()) < 4.0 / math.sqrt(N), n.mean()
    assert abs(n.var() - 1.0) < 4.0 * math.sqrt(2.0 / N), n.var()
    assert np.abs(n).max() <= math.sqrt(48.0 * math.log(2.0))
    assert np.all(np.abs(n) <= r + 1e-12)
    # a pair shares its word: the stream from an even offset is the same stream
    n2, _ = ref.normals(12345, 64, first=1000)
    assert np.array_equal(n2, n[1000:1064])


def test_restatement_drop_rate():
    p, B, V = 0.3, 1 << 12, 16
    _, drew = ref.dropped_rows(777, B, V, p)
    N = B * V
    assert N == 1 << 16
    assert abs(drew.mean() - p) < 4.0 * math.sqrt(p * (1 - p) / N), drew.mean()
    dropped, _ = ref.dropped_rows(777, B, V, p)
    assert (~dropped).any(axis=1).all()


def test_restatement_fallback_keeps_one_lead():
    B, V = 4096, 3
    dropped, drew = ref.dropped_rows(5, B, V, 0.5)
    all3 = drew.all(axis=1)
    assert all3.sum() > 300                                   # ~ B / 8
    assert (dropped[all3].sum(axis=1) == V - 1).all()
    assert np.array_equal(dropped[~all3], drew[~all3])
    kept = np.argmin(dropped[all3], axis=1)
    assert set(kept.tolist()) == {0, 1, 2}


def test_restatement_terms_and_crop():
    rng = np.random.default_rng(0)
    x = rng.random((2, 3, 16), dtype=np.float32)
    rois = np.zeros((2, 7, 2), np.int64)
    rois[:, -1, 0] = (5, 99)
    y, dropped, M = ref.augment(x, rois, 9, noise_std=0.1, wander_amp=0.2, hum_amp=0.05)
    assert not dropped.any()
    assert np.array_equal(y[0, :, 5:], x[0, :, 5:].astype(np.float64)) and np.all(y[0, :, :5] != x[0, :, :5])
    assert np.all(y[1] != x[1]) and np.all(np.abs(y - x) <= M - np.abs(x) + 1e-12)
    y2, _, _ = ref.augment(x, rois, 9, noise_std=0.1, wander_amp=0.2, hum_amp=0.05, crop=False)
    assert np.all(y2 != x) and np.array_equal(y2[1], y[1])
    y3, d3, M3 = ref.augment(x, rois, 9)
    assert np.array_equal(y3, x.astype(np.float64)) and np.array_equal(M3, np.abs(x).astype(np.float64))


def test_ops_augment_checks_its_arguments_before_the_library(monkeypatch):
    from electrocardio_panorama_amd import _lib, augment, ops

    def touched():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", touched)
    aug = augment.from_cfg(_cfg(aug_noise_std=0.1))
    x = torch.zeros(2, 3, 8)
    rois = torch.zeros(2, 7, 2, dtype=torch.int64)
    assert ops.augment(x, rois, None) is x                    # off: the tensor itself
    assert ops.augment(x.double(), None, None).dtype == torch.float64
    with pytest.raises(TypeError, match="float32"):
        ops.augment(x.double(), rois, aug)
    with pytest.raises(ValueError, match=r"\[B, V, L\]"):
        ops.augment(x[0], rois, aug)
    with pytest.raises(ValueError, match="contiguous"):
        ops.augment(x.transpose(0, 1), rois, aug)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.augment(torch.zeros(2, 3, 6), rois, aug)
    with pytest.raises(TypeError, match="integer"):
        ops.augment(x, rois.float(), aug)
    with pytest.raises(TypeError, match="integer"):
        ops.augment(x, None, aug)
    with pytest.raises(ValueError, match="rois"):
        ops.augment(x, rois[:1], aug)
    with pytest.raises(ValueError, match="rois"):
        ops.augment(x, torch.zeros(2, 7, 3, dtype=torch.int64), aug)
    with pytest.raises(ValueError, match="out"):
        ops.augment(x, rois, aug, out=torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="out of place"):
        ops.augment(x, rois, aug, out=x)
    with pytest.raises(ValueError, match="seed_dev"):
        ops.augment(x, rois, aug, seed_dev=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.augment(x, rois, aug)                             # a CPU tensor, everything else right: still in front of the library


def test_model_and_stepper_default_to_no_augmentation():
    from electrocardio_panorama_amd.graph import GraphedTrainStep
    from electrocardio_panorama_amd.network import build_model
    cfg = _cfg(lead_num=3)
    cfg.MODEL.model = "model_nefnet"
    m = build_model(cfg)
    assert m.augment is None
    st = GraphedTrainStep(m, cfg)
    assert st.augment is None and st.data_aug is None
    cfg.DATA.aug_lead_drop = 0.25
    assert GraphedTrainStep(m, cfg).augment.lead_drop == 0.25
