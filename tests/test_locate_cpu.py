"""CPU: the panorama search that locates a lead's viewing angle (Model_nefnet.locate) -- the fp64 restatement tests/locate_ref.py pinned
to tests/corr_ref.py's r and to a literal loop, the grid's index and step conventions, the best rule on hand-made tables, the fp32
candidate formula, the C-ABI entries in the header, the binding table and the library, their argument checks (no GPU work), the config
keys and the ValueErrors, and the precondition of the device tests' 'corr' bar on the device tests' inputs."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import corr_ref
import locate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nef_locate_score", "nef_locate_score_args_bytes", "nef_locate_best", "nef_locate_best_args_bytes", "nef_locate_cands",
           "nef_locate_cands_args_bytes")
INF, NAN = float("inf"), float("nan")


class Cfg(dict):
    __getattr__ = dict.__getitem__


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("L,ends", [(2, [2, 2]), (13, [13, 7]), (40, [33, 1]), (500, [298, 0]), (512, [440, 512])])
def test_corr_score_is_one_minus_corr_refs_r(L, ends):
    pred, obs = locate_ref.case(3, 5, 512)
    pred, obs = pred[:, :, :L], obs[:, :, :L]
    got = locate_ref.scores(pred, obs, ends, "corr")
    assert got.shape == (2, 3, 5)
    for b in range(2):
        for r in range(3):
            for a in range(5):
                want = corr_ref.corr_rows(torch.from_numpy(pred[b, a:a + 1].copy()), torch.from_numpy(obs[b, r:r + 1].copy()), corr_ref.EPS,
                                          [ends[b]])[0]
                if want is None:
                    assert got[b, r, a] == INF
                else:
                    assert abs(got[b, r, a] - (1.0 - float(want))) <= 1e-12, (b, r, a)
    # the grouped mapping is the same numbers: candidate a against row a // G
    grouped = locate_ref.scores(pred[:, :3], obs, ends, "corr", group=1)
    assert grouped.shape == (2, 3, 1)
    for r in range(3):
        assert np.array_equal(grouped[:, r, 0], got[:, r, r])


@pytest.mark.parametrize("L,ends", [(1, [1, 0]), (7, [7, 3]), (257, [-2, 257])])
def test_mse_score_is_the_literal_loop(L, ends):
    pred, obs = locate_ref.case(3, 5, 512)
    pred, obs = pred[:, :, :L], obs[:, :, :L]
    n = corr_ref.row_ends(corr_ref.rois_of(ends), 2, L)
    got = locate_ref.scores(pred, obs, n, "mse")
    for b in range(2):
        for r in range(3):
            for a in range(5):
                want = locate_ref.mse_loop(pred[b, a], obs[b, r], n[b])
                assert got[b, r, a] == want or abs(got[b, r, a] - want) <= 1e-13 * want, (b, r, a)
    assert np.isinf(got[[k for k in range(2) if n[k] < 1]]).all()


def test_identical_rows_score_exactly_zero_and_nan_counts_as_inf():
    pred, obs = locate_ref.case(1, 5, 512)
    for mode in ("mse", "corr"):
        assert float(locate_ref.scores(obs, obs, [512, 300], mode).max()) == 0.0
    bad = pred.copy()
    bad[0, 2, 5] = np.nan
    for mode in ("mse", "corr"):
        s = locate_ref.scores(bad, obs, [512, 512], mode)
        assert s[0, 0, 2] == INF and np.isfinite(np.delete(s[0, 0], 2)).all() and np.isfinite(s[1]).all()
    # no gain or offset of the observed lead changes 'corr' (beyond eps' share)
    a = locate_ref.scores(pred, obs, [512, 512], "corr")
    b = locate_ref.scores(pred, np.float32(0.5) * obs + np.float32(0.2), [512, 512], "corr")
    assert float(np.abs(a - b).max()) < 1e-5


# ------------------------------------------------------------------------------------------------ grid
def test_grid_index_and_step_conventions():
    from electrocardio_panorama_amd import locate, synth
    g = locate.Grid()
    assert (g.n1, g.n2, g.size) == (9, 19, 171)
    d1, d2 = g.steps
    assert abs(d1 - math.radians(15)) < 1e-15 and abs(d2 - math.radians(10)) < 1e-15
    th = g.thetas()
    assert th.dtype == np.float32 and th.shape == (171, 2)
    for i, k in ((0, 0), (0, 18), (3, 7), (8, 18)):
        assert g.index(i, k) == i * 19 + k
        assert th[g.index(i, k), 0] == np.float32(g.lo1 + i * d1) and th[g.index(i, k), 1] == np.float32(g.lo2 + k * d2)
    # the default range is the span of the nominal lead table
    assert abs(synth.LEAD_THETA[:, 0].min() - g.lo1) < 1e-12 and abs(synth.LEAD_THETA[:, 0].max() - g.hi1) < 1e-12
    assert abs(synth.LEAD_THETA[:, 1].min() - g.lo2) < 1e-12 and abs(synth.LEAD_THETA[:, 1].max() - g.hi2) < 1e-12
    # n == 1 pins the axis at lo with step 0
    p = locate.Grid(1, 4, 0.5, 2.0, -1.0, 2.0)
    assert p.steps == (0.0, 1.0) and p.thetas().tolist() == [[0.5, -1.0], [0.5, 0.0], [0.5, 1.0], [0.5, 2.0]]
    assert locate.Grid(1, 1).check().thetas().shape == (1, 2)
    # the accepted spellings
    assert locate.as_grid(None) == g and locate.as_grid((4, 6)) == locate.Grid(4, 6)
    assert locate.as_grid(locate.Grid(4, 6, 0.0, 1.0, -1.0, 1.0)) == locate.Grid(4, 6, 0.0, 1.0, -1.0, 1.0)
    # steps halve exactly, in fp32
    s = locate.level_steps(g, 3)
    assert [type(v) for v in s[0]] == [np.float32, np.float32]
    assert s[0] == (np.float32(d1) / 2, np.float32(d2) / 2) and s[2] == (np.float32(d1) / 8, np.float32(d2) / 8)
    assert locate.level_steps(g, 0) == []


# ------------------------------------------------------------------------------------------------ best rule, candidates
def test_best_rule_on_hand_made_tables():
    c = np.arange(12, dtype=np.float32).reshape(6, 2)
    best = locate_ref.best
    assert best([3.0, 1.0, 2.0, 1.0, 5.0, 1.0], c) == (1.0, (2.0, 3.0), 1)                       # ties: the earliest
    assert best([INF, 4.0, NAN, 4.0, INF, 9.0], c) == (4.0, (2.0, 3.0), 1)                        # inf and NaN never win
    assert best([NAN, INF, 7.0, INF, NAN, INF], c, index_base=100) == (7.0, (4.0, 5.0), 102)
    s, t, i = best([INF, NAN, INF, INF, NAN, INF], c)
    assert s == INF and i == -1 and math.isnan(t[0]) and math.isnan(t[1])                        # no finite score
    # merging: only a strictly lower score replaces the running best
    run = (2.0, (np.float32(9), np.float32(9)), 7)
    assert best([3.0, 2.0, 2.5, 9.0, 9.0, 9.0], c, run, index_base=10) == run
    assert best([3.0, 1.5, 2.5, 1.5, 9.0, 9.0], c, run, index_base=10) == (1.5, (2.0, 3.0), 11)
    assert best([3.0, 1.5, 2.5, 1.5, 9.0, 9.0], c, run, keep_index=True) == (1.5, (2.0, 3.0), 7)
    # a pair without a finite level-0 score stays at -1 on every later level
    none = (INF, (np.float32(NAN), np.float32(NAN)), -1)
    out = best([0.5] * 6, c, none, keep_index=True)
    assert out[0] == INF and out[2] == -1
    assert best([0.5] * 6, c, none, index_base=6) == (0.5, (0.0, 1.0), 6)                        # (level 0, a later chunk: it may still win)
    bs, bt, bi = locate_ref.best_table(np.array([[[3.0, 1.0, 1.0], [INF, NAN, INF]]]), c[:3])
    assert bs.tolist() == [[1.0, INF]] and bi.tolist() == [[1, -1]] and bt[0, 0].tolist() == [2.0, 3.0] and np.isnan(bt[0, 1]).all()


def test_candidate_formula():
    bt = np.array([[[1.25, -0.5], [np.nan, np.nan]]], dtype=np.float32)
    bi = np.array([[4, -1]])
    s1, s2 = np.float32(0.1308997), np.float32(0.08726646)
    c = locate_ref.level_cands(bt, bi, s1, s2, 2, (np.float32(1.0471976), np.float32(-1.5707964)))
    assert c.dtype == np.float32 and c.shape == (1, 2 * 25, 2)
    for r, centre in ((0, bt[0, 0]), (1, np.array([1.0471976, -1.5707964], dtype=np.float32))):
        for i in range(5):
            for k in range(5):
                want = (np.float32(centre[0] + np.float32(np.float32(i - 2) * s1)), np.float32(centre[1] + np.float32(np.float32(k - 2) * s2)))
                assert tuple(c[0, r * 25 + i * 5 + k]) == want
        assert tuple(c[0, r * 25 + 12]) == tuple(centre)                                         # the middle candidate is the centre itself


# ------------------------------------------------------------------------------------------------ precondition of the device bar
@pytest.mark.parametrize("R,A,L", locate_ref.SHAPES, ids=locate_ref.IDS)
def test_the_device_tests_inputs_keep_the_corr_bound_small(R, A, L):
    """tests/test_locate_gpu.py holds the 'corr' scores to 3 delta / min(vx + eps, vy + eps) per row; that bar means something only where
    it is small: at most 1e-8 on every counted row of every input, both mappings."""
    pred, obs = locate_ref.case(R, A, L)
    for ends in locate_ref.end_variants(L):
        n = locate_ref.row_ends(None if ends is None else corr_ref.rois_of(ends), locate_ref.B, L)
        s, bound = locate_ref.scores(pred, obs, n, "corr", with_bound=True)
        counted = np.isfinite(s)
        assert counted.all(axis=(1, 2)).tolist() == [v >= 2 for v in n]
        if counted.any():
            print(f"R={R} A={A} L={L} ends={ends}: largest bound {bound[counted].max():.2e}, scores in [{s[counted].min():.3g}, {s[counted].max():.3g}]")
            assert float(bound[counted].max()) <= locate_ref.BOUND_CAP, (ends, float(bound[counted].max()))
            assert float(bound[counted].min()) > 0.0
    if L >= 64:          # r near 0 on the independent candidates, near 1 on the blended ones
        s = locate_ref.scores(pred, obs, [L] * locate_ref.B, "corr")
        assert float(np.abs(s[:, :, 0::2] - 1.0).max()) < 0.6
        for a in range(1, A, 2):
            assert float(s[:, a % R, a].max()) < 0.05


# ------------------------------------------------------------------------------------------------ C ABI
def _fields(hdr, name):
    body = hdr[hdr.index("typedef struct " + name):hdr.index("} " + name + ";")]
    return re.findall(r"(\w+);\s*/\*", body) + []


def test_header_binding_and_library_agree():
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    build.build(verbose=False)
    assert "locate.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "nefnet_hip.h")).read()
    for fn in ("score", "best", "cands"):
        assert re.search(r"\bint nef_locate_" + fn + r"\s*\(\s*const nef_locate_" + fn + r"_args\s*\*\s*a,\s*nef_stream_t stream\s*\)", hdr)
        assert re.search(r"\bsize_t nef_locate_" + fn + r"_args_bytes\s*\(\s*void\s*\)", hdr)
    for name, mirror in (("nef_locate_score_args", _lib.LocateScoreArgs), ("nef_locate_best_args", _lib.LocateBestArgs),
                         ("nef_locate_cands_args", _lib.LocateCandsArgs)):
        body = hdr[hdr.index("typedef struct " + name):hdr.index("} " + name + ";")]
        declared = re.findall(r"^\s+[\w \*]+?\b(\w+);", body, flags=re.M)
        assert declared == [n for n, _ in mirror._fields_], name
    L = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert L.nef_abi_version() == 22                    # additions: the number stays
    assert ctypes.sizeof(_lib.LocateScoreArgs) == L.nef_locate_score_args_bytes() == 120
    assert ctypes.sizeof(_lib.LocateBestArgs) == L.nef_locate_best_args_bytes() == 88
    assert ctypes.sizeof(_lib.LocateCandsArgs) == L.nef_locate_cands_args_bytes() == 56
    from electrocardio_panorama_amd import locate, ops
    assert ops.LOCATE_MODES == {"mse": 0, "corr": 1} and tuple(ops.LOCATE_MODES) == locate.SCORES
    assert int(re.search(r"#define NEF_LOCATE_SEG (\d+)", hdr).group(1)) == 1024


def test_a_struct_of_another_size_is_rejected(monkeypatch):
    from electrocardio_panorama_amd import _lib
    from electrocardio_panorama_amd.csrc import build
    build.build(verbose=False)

    class Short(ctypes.Structure):
        _fields_ = _lib.LocateScoreArgs._fields_[:-2]

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LocateScoreArgs", Short)
    with pytest.raises(_lib.NefLibraryError, match="nef_locate_score_args is 120 bytes"):
        _lib.load()


def _score_args(**kw):
    from electrocardio_panorama_amd import _lib
    a = dict(pred=64, obs=64, rois=None, scores=64, pred_bs=26 * 512, pred_as=512, obs_bs=3 * 512, obs_rs=512, sc_bs=3 * 26, sc_rs=26,
             col_off=0, eps=1e-8, B=2, A=26, R=3, L=512, mode=1, group=0)
    a.update(kw)
    return _lib.LocateScoreArgs(**a)


def _best_args(**kw):
    from electrocardio_panorama_amd import _lib
    a = dict(scores=64, cands=64, best_score=64, best_theta=64, best_index=64, sc_bs=3 * 26, sc_rs=26, index_base=0, B=2, R=3, A=26,
             per_pair=0, init=1, keep_index=0)
    a.update(kw)
    return _lib.LocateBestArgs(**a)


def _cands_args(**kw):
    from electrocardio_panorama_amd import _lib
    a = dict(best_theta=64, best_index=64, cands=64, s1=0.1, s2=0.05, ph1=1.0, ph2=-1.5, B=2, R=3, radius=2, reserved0=0)
    a.update(kw)
    return _lib.LocateCandsArgs(**a)


def test_entries_reject_bad_arguments_without_touching_the_gpu():
    """Every check sits in front of the launch: nothing is launched and no address is read (non-NULL, never dereferenced pointers)."""
    from electrocardio_panorama_amd import _lib
    L = _lib.load()
    score = lambda **kw: L.nef_locate_score(ctypes.byref(_score_args(**kw)), None)       # noqa: E731
    best = lambda **kw: L.nef_locate_best(ctypes.byref(_best_args(**kw)), None)          # noqa: E731
    cands = lambda **kw: L.nef_locate_cands(ctypes.byref(_cands_args(**kw)), None)       # noqa: E731
    assert L.nef_locate_score(None, None) == -2 and L.nef_locate_best(None, None) == -2 and L.nef_locate_cands(None, None) == -2
    for key in ("pred", "obs", "scores"):
        assert score(**{key: None}) == -2, key                                           # NEF_E_NULL
    for key in ("B", "A", "R", "L"):
        for bad in (0, -1):
            assert score(**{key: bad}) == -1, (key, bad)                                 # NEF_E_SHAPE
    assert score(group=8) == -1 and score(group=9) == -1 and score(group=-1) == -1       # A = 26 is not 3 x G
    assert score(A=24, group=7) == -1
    for bad in (2, -1, 7):
        assert score(mode=bad) == -1, bad
    for mode in (0, 1):
        for bad in (0.0, -1e-8, math.nan, math.inf):
            assert score(mode=mode, eps=bad) == -1, (mode, bad)
    for key in ("pred_bs", "pred_as", "obs_bs", "obs_rs", "sc_bs", "sc_rs", "col_off"):
        assert score(**{key: -1}) == -1, key
    assert score(B=1 << 30, A=26) == -1                                                  # B * ceil(A / 4) blocks
    assert score(pred=None, B=0) == -2                                                   # a NULL pointer wins over a bad shape
    for key in ("scores", "cands", "best_score", "best_theta", "best_index"):
        assert best(**{key: None}) == -2, key
    for key in ("B", "R", "A"):
        for bad in (0, -1):
            assert best(**{key: bad}) == -1, (key, bad)
    for key in ("sc_bs", "sc_rs", "index_base"):
        assert best(**{key: -1}) == -1, key
    assert best(B=1 << 16, R=1 << 15) == -1 and best(scores=None, A=0) == -2
    for key in ("best_theta", "best_index", "cands"):
        assert cands(**{key: None}) == -2, key
    for key in ("B", "R"):
        for bad in (0, -1):
            assert cands(**{key: bad}) == -1, (key, bad)
    assert cands(radius=-1) == -1 and cands(radius=17) == -1
    for key in ("s1", "s2", "ph1", "ph2"):
        for bad in (math.nan, math.inf, -math.inf):
            assert cands(**{key: bad}) == -1, (key, bad)
    assert cands(B=1 << 20, R=1 << 10, radius=2) == -1 and cands(cands=None, B=0) == -2


def test_a_library_without_the_entries_is_rejected(monkeypatch):
    import _ctypes
    from electrocardio_panorama_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", _ctypes.__file__)
    with pytest.raises(_lib.NefLibraryError, match="rebuild"):
        _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES


# ------------------------------------------------------------------------------------------------ config, ValueErrors
def test_config_defaults_are_off():
    from electrocardio_panorama_amd import locate
    from electrocardio_panorama_amd.config import get_defaults
    cfg = get_defaults()
    s = cfg.SOLVER
    assert s.locate_eval is False and list(s.locate_grid) == [9, 19] and [list(r) for r in s.locate_range_deg] == [[60, 180], [-90, 90]]
    assert s.locate_score == "corr" and s.locate_levels == 3 and s.locate_radius == 2
    assert locate.from_cfg(cfg) is None
    cfg.merge_from_list(["SOLVER.locate_eval", "True"])
    kw = locate.from_cfg(cfg)
    g = locate.Grid()
    assert (kw["grid"].n1, kw["grid"].n2) == (9, 19) and kw["score"] == "corr" and kw["levels"] == 3 and kw["radius"] == 2 and kw["eps"] == 1e-8
    assert all(abs(a - b) < 1e-12 for a, b in zip(kw["grid"][2:], g[2:]))
    # off: the other keys are not looked at
    off = Cfg(SOLVER=Cfg(locate_eval=False, locate_grid="bad", locate_score="nope"))
    assert locate.from_cfg(off) is None and locate.from_cfg(Cfg(SOLVER=Cfg())) is None


@pytest.mark.parametrize("kw,match", [
    (dict(grid=(0, 4)), "n1"), (dict(grid=(4, -1)), "n2"), (dict(grid=(2.5, 4)), "n1"), (dict(grid="abc"), "grid"),
    (dict(grid=("4, 6", (1.0, 0.0, 0.0, 1.0))), "theta1"), (dict(grid=("4, 6", (0.0, 1.0, 1.0, 1.0))), "theta2"),
    (dict(grid=("4, 6", (0.0, math.inf, 0.0, 1.0))), "finite"), (dict(grid=(2048, 2048)), "2\\^20"),
    (dict(score="l1"), "score"), (dict(score=None), "score"),
    (dict(levels=-1), "levels"), (dict(levels=2.0), "levels"), (dict(levels=25), "levels"), (dict(levels=True), "levels"),
    (dict(radius=-1), "radius"), (dict(radius=17), "radius"), (dict(radius=1.5), "radius"), (dict(radius=0, levels=1), "radius"),
    (dict(eps=0.0), "eps"), (dict(eps=-1e-8), "eps"), (dict(eps=math.nan), "eps"), (dict(eps=math.inf), "eps"), (dict(eps="x"), "eps"),
])
def test_bad_settings_raise(kw, match):
    from electrocardio_panorama_amd import locate
    if "grid" in kw and kw["grid"][0] == "4, 6":            # a Grid with a bad range
        kw = dict(grid=locate.Grid(4, 6, *kw["grid"][1]))
    with pytest.raises(ValueError, match=match):
        locate.check_settings(**kw)
    if "eps" not in kw:
        keys = dict(locate_eval=True)
        if "grid" in kw and type(kw["grid"]) is tuple:
            keys["locate_grid"] = list(kw["grid"])
        elif "grid" in kw:
            return
        for k in ("score", "levels", "radius"):
            if k in kw:
                keys["locate_" + k] = kw[k]
        with pytest.raises(ValueError, match=match):
            locate.from_cfg(Cfg(SOLVER=Cfg(**keys)))


def test_settings_that_are_fine():
    from electrocardio_panorama_amd import locate
    st = locate.check_settings()
    assert st.grid == locate.Grid() and st.score == "corr" and st.levels == 3 and st.radius == 2
    assert locate.check_settings((4, 6), "mse", 0, 0, 1e-6).levels == 0
    assert locate.check_settings(locate.Grid(1, 1), "mse", 2, 1).grid.size == 1


def test_model_locate_raises_before_any_device_work():
    """CPU tensors: the ValueErrors come before the first launch (which would reject them)."""
    from electrocardio_panorama_amd.network import build_model
    cfg = Cfg(MODEL=Cfg(model="model_nefnet", theta_L=1, loss="v1", resume=""), DATA=Cfg(lead_num=3, noise=False))
    m = build_model(cfg).float().train()
    x, th, rois, obs = torch.zeros(2, 3, 64), torch.zeros(2, 3, 2), torch.zeros(2, 7, 2, dtype=torch.int64), torch.zeros(2, 64)
    with pytest.raises(ValueError, match="crop"):
        m.locate(x, th, None, obs)                          # crop defaults to True
    with pytest.raises(ValueError, match="score"):
        m.locate(x, th, rois, obs, score="l1")
    with pytest.raises(ValueError, match="levels"):
        m.locate(x, th, rois, obs, levels=-1)
    with pytest.raises(ValueError, match="radius"):
        m.locate(x, th, rois, obs, radius=40)
    with pytest.raises(ValueError, match="n1"):
        m.locate(x, th, rois, obs, grid=(0, 3))
    with pytest.raises(ValueError, match="observed"):
        m.locate(x, th, rois, torch.zeros(2, 32))
    with pytest.raises(ValueError, match="observed"):
        m.locate(x, th, rois, torch.zeros(3, 2, 64))
    with pytest.raises(ValueError, match="chunk"):
        m.locate(x, th, rois, obs, chunk=0)
    m.panorama_dtype = "bf16"
    with pytest.raises(ValueError, match="panorama_dtype"):
        m.locate(x, th, rois, obs)
    assert m.training                                       # the mode it was in


def test_solver_locate_is_one_rank_only(monkeypatch):
    import torch.distributed as dist
    from electrocardio_panorama_amd.solver.solver import Solver
    s = Solver.__new__(Solver)
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="locate_eval"):
        s.locate([])


def test_val_net_has_the_locate_switch(monkeypatch):
    from electrocardio_panorama_amd import val_net
    seen = {}
    monkeypatch.setattr(val_net, "main", lambda cfg, epoch=-1: seen.update(on=bool(cfg.SOLVER.locate_eval), epoch=epoch))
    saved = (val_net.cfg.SOLVER.locate_eval, val_net.cfg.desc, val_net.cfg.output_dir)
    try:
        val_net.run(["--locate", "--epoch", "3"])
        assert seen == dict(on=True, epoch=3)
        val_net.cfg.SOLVER.locate_eval = False
        val_net.run([])
        assert seen == dict(on=False, epoch=-1)
    finally:
        val_net.cfg.SOLVER.locate_eval, val_net.cfg.desc, val_net.cfg.output_dir = saved
