"""CPU: several target views per train step (SOLVER.train_views) -- the key's validation, the per-step view draw, the train collate and the
argument checks of the nef_copy_many C-ABI entry (no GPU work)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(*pairs):
    from electrocardio_panorama_amd.config import get_defaults
    cfg = get_defaults()
    cfg.merge_from_list(list(pairs))
    return cfg


# ------------------------------------------------------------------------------------------------ the key
def test_config_default_is_off():
    from electrocardio_panorama_amd import views
    cfg = _cfg()
    assert cfg.SOLVER.train_views == 1 and views.train_views(cfg) == 1
    assert views.train_views(_cfg("SOLVER.train_views", "4")) == 4
    old = _cfg()
    del old.SOLVER["train_views"]                          # a config written before the key existed
    assert views.train_views(old) == 1


@pytest.mark.parametrize("bad", [0, -1, -7])
def test_train_views_below_one_raises(bad):
    from electrocardio_panorama_amd import views
    with pytest.raises(ValueError, match="train_views"):
        views.train_views(_cfg("SOLVER.train_views", bad))


def test_noise_with_views_raises():
    from electrocardio_panorama_amd import views
    with pytest.raises(ValueError, match="DATA.noise"):
        views.train_views(_cfg("SOLVER.train_views", 2, "DATA.noise", True))
    assert views.train_views(_cfg("SOLVER.train_views", 1, "DATA.noise", True)) == 1       # off: noise is the reference's


def test_more_views_than_supervised_raises():
    from electrocardio_panorama_amd import views
    # the shipped scheme: 3 inputs, IIv2v5_v4I_372 -> 9 rest views, the last two unsupervised
    cfg = _cfg("DATA.lead_num", 3, "DATA.super_mode", "IIv2v5_v4I_372", "DATA.train_data_mode", "input_fix")
    assert views.planned_views(cfg) == (9, 7) and views.supervised_views(cfg, 9) == 7
    with pytest.raises(ValueError, match="train_views"):
        views.draw_views(0, 0, 0, 8, views.supervised_views(cfg, 9))
    with pytest.raises(ValueError, match="train_views"):
        views.check_views(8, 7)
    views.check_views(7, 7)
    # synthetic batches: every rest view is supervised
    assert views.supervised_views(_cfg("DATA.synthetic", True), 9) == 9


def test_supervised_count_leaves_the_global_stream_alone():
    from electrocardio_panorama_amd import views
    cfg = _cfg("DATA.lead_num", 3, "DATA.super_mode", "IIv2v5_v4I_372", "DATA.train_data_mode", "input_fix")   # (its lead plan draws)
    random.seed(11)
    state = random.getstate()
    views.supervised_views(cfg, 9), views.planned_views(cfg)
    assert random.getstate() == state


# ------------------------------------------------------------------------------------------------ the draw
def test_draw_is_a_function_of_seed_epoch_index_only():
    from electrocardio_panorama_amd.views import draw_views
    random.seed(5)
    a = [draw_views(3, e, i, 3, 7) for e in range(3) for i in range(20)]
    random.seed(99)
    [random.random() for _ in range(17)]
    b = [draw_views(3, e, i, 3, 7) for e in range(3) for i in range(20)]
    assert a == b
    # ... and really of each of the three: over 20 batches the draws differ somewhere
    assert [draw_views(4, 0, i, 3, 7) for i in range(20)] != a[:20]
    assert a[:20] != a[20:40]
    assert len({tuple(d) for d in a[:20]}) > 1


def test_draw_leaves_the_global_stream_alone():
    from electrocardio_panorama_amd.views import draw_views
    random.seed(1)
    state = random.getstate()
    for i in range(10):
        draw_views(0, 0, i, 2, 7)
        draw_views(0, 0, i, 7, 7)
    assert random.getstate() == state


@pytest.mark.parametrize("Q,S", [(2, 7), (3, 7), (6, 7), (2, 2), (4, 9)])
def test_draw_is_sorted_without_repeats_from_the_first_S(Q, S):
    from electrocardio_panorama_amd.views import draw_views
    seen = set()
    for i in range(200):
        d = draw_views(7, 1, i, Q, S)
        assert len(d) == Q and d == sorted(set(d)) and 0 <= d[0] and d[-1] < S
        seen.update(d)
    assert seen == set(range(S))                           # every supervised view is reachable


def test_draw_of_all_views_is_the_identity():
    from electrocardio_panorama_amd.views import draw_views
    for S in (2, 5, 7):
        assert all(draw_views(s, e, i, S, S) == list(range(S)) for s in range(2) for e in range(2) for i in range(5))


def test_select_views_is_view_major():
    from electrocardio_panorama_amd.views import select_views
    rv = torch.arange(2 * 5 * 4, dtype=torch.float64).view(2, 5, 4)
    rt = torch.arange(2 * 5 * 2, dtype=torch.float32).view(2, 5, 2)
    tv, th = select_views(rv, rt, [1, 3])
    assert tv.shape == (2, 2, 1, 4) and th.shape == (2, 2, 2) and tv.dtype == torch.float32 and tv.is_contiguous() and th.is_contiguous()
    for k, v in enumerate([1, 3]):
        assert torch.equal(tv[k, :, 0], rv[:, v].float()) and torch.equal(th[k], rt[:, v])


# ------------------------------------------------------------------------------------------------ the loader
def _items(n=3, n_rest=9):
    rng = np.random.default_rng(0)
    return [{"data": rng.random((3, 8), dtype=np.float32), "rois": np.zeros((7, 2), np.int64), "input_theta": rng.random((3, 2), dtype=np.float32),
             "target_view": rng.random(8, dtype=np.float32), "target_theta": rng.random(2, dtype=np.float32), "id": f"r{i}",
             "ori_data": rng.random((12, 8)), "rest_view": rng.random((n_rest, 8)), "rest_theta": rng.random((n_rest, 2), dtype=np.float32),
             "noise": rng.random(8, dtype=np.float32), "unsupervision_lead_name": [5, 0]} for i in range(n)]


def test_collate_train_ships_the_rest_views_only_with_the_key_on():
    from electrocardio_panorama_amd.train_net import _TRAIN_FIELDS, _collate_train
    items = _items()
    off = _collate_train(items)
    assert set(off) == set(_TRAIN_FIELDS) == {"data", "rois", "input_theta", "target_view", "target_theta", "noise", "rest_theta"}
    on = _collate_train(items, rest_views=7)
    assert set(on) == set(off) | {"rest_view"}
    assert on["rest_view"].dtype == torch.float32 and on["rest_view"].shape == (3, 7, 8)
    assert np.array_equal(on["rest_view"].numpy(), np.stack([it["rest_view"][:7] for it in items]).astype(np.float32))
    for k in off:
        assert torch.equal(on[k], off[k])


def test_synthetic_loader_carries_float32_rest_views():
    from electrocardio_panorama_amd.train_net import SyntheticLoader
    meta = next(iter(SyntheticLoader(_cfg("DATA.lead_num", 3), batch_size=2, n_batches=1, length=64)))
    assert meta["rest_view"].dtype == torch.float32 and meta["rest_view"].shape == (2, 9, 64) and meta["rest_theta"].shape == (2, 9, 2)


# ------------------------------------------------------------------------------------------------ the loss's row limit
def test_ssim_rows_of_a_multi_view_step_are_limited():
    from electrocardio_panorama_amd.network.loss.losses import check_view_rows
    check_view_rows(4, 16383)
    with pytest.raises(ValueError, match=r"train_views.*ssim_factor|ssim_factor.*train_views"):
        check_view_rows(4, 16384)


# ------------------------------------------------------------------------------------------------ the C entry
def test_header_declares_the_entry_and_binding_has_it():
    from electrocardio_panorama_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    assert re.search(r"\bint nef_copy_many\s*\(\s*const float\s*\*\s*const\s*\*\s*srcs,\s*float\s*\*\s*const\s*\*\s*dsts,\s*const int64_t\s*\*\s*sizes,"
                     r"\s*int n,\s*int accumulate,\s*nef_stream_t stream\s*\)", hdr)
    doc = hdr[:hdr.index("int nef_copy_many")].rsplit("/*", 1)[1]
    assert "HOST" in doc and "+=" in doc and "OVERLAPPING SEGMENTS ARE NOT SUPPORTED" in doc
    L = _lib.load()
    assert hasattr(L, "nef_copy_many") and len(_lib.SIGNATURES["nef_copy_many"][1]) == 6
    assert L.nef_abi_version() == 22          # additive
    assert callable(ops.copy_many)


def _call(n, srcs="ok", dsts="ok", sizes="ok", accumulate=0, vals=None, sptrs=None, dptrs=None):
    """nef_copy_many with a NULL stream and (non-NULL, never dereferenced) device addresses."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    k = max(n, 1) if vals is None else len(vals)
    s = (ctypes.c_void_p * k)(*(sptrs if sptrs is not None else [64] * k)) if srcs == "ok" else None
    d = (ctypes.c_void_p * k)(*(dptrs if dptrs is not None else [4096] * k)) if dsts == "ok" else None
    z = (ctypes.c_int64 * k)(*(vals if vals is not None else [4] * k)) if sizes == "ok" else None
    return L.nef_copy_many(s, d, z, n, accumulate, None)


def test_nef_copy_many_rejects_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the first launch, so nothing is launched and no address is read."""
    assert _call(2, srcs=None) == -2                       # NEF_E_NULL
    assert _call(2, dsts=None) == -2
    assert _call(2, sizes=None) == -2
    assert _call(2, vals=[4, 4], sptrs=[64, None]) == -2   # a NULL pointer of a non-empty segment
    assert _call(2, vals=[4, 4], dptrs=[None, 4096]) == -2
    assert _call(-1) == -1                                 # NEF_E_SHAPE
    assert _call(-1, srcs=None, dsts=None, sizes=None) == -1
    assert _call(2, vals=[4, -1]) == -1
    assert _call(2, accumulate=2) == -1 and _call(2, accumulate=-1) == -1
    # ... also behind the 64th segment, in front of what would be the first launch
    assert _call(70, vals=[4] * 69 + [-3]) == -1
    assert _call(70, vals=[4] * 70, sptrs=[64] * 69 + [None]) == -2
    assert _call(70, vals=[4] * 70, dptrs=[4096] * 69 + [None]) == -2
    # n == 0: nothing to do, whatever the pointers are
    assert _call(0) == 0 and _call(0, srcs=None, dsts=None, sizes=None) == 0
    assert _call(0, accumulate=1) == 0


def test_model_rejects_a_3d_query_outside_the_train_phase_signature():
    """The rejection sits in front of any device work (Model_nefnet2 and the other phases take [B, 2])."""
    from electrocardio_panorama_amd import engine
    x, th, q3, rois = torch.zeros(2, 1, 64), torch.zeros(2, 1, 2), torch.zeros(2, 2, 2), torch.zeros(2, 7, 2, dtype=torch.int64)
    for phase in ("val", "test", "gen"):
        with pytest.raises(ValueError, match="query_theta"):
            engine.forward({}, {}, x, th, q3, rois, phase=phase)
    with pytest.raises(ValueError, match="query_theta"):
        engine.forward2({}, {}, x, th, q3, rois, phase="train")
    with pytest.raises(ValueError, match="query_theta"):
        engine.forward({}, {}, x, th, torch.zeros(2, 3, 2), rois, phase="train")          # [Q, B', 2] with B' != B
