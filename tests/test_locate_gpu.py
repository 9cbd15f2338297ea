"""The panorama search that locates a lead's viewing angle, on the device (nef_locate_score / nef_locate_best / nef_locate_cands,
ops.locate_*, engine.locate, Model_nefnet.locate, Solver.locate): the kernels against the fp64 restatement tests/locate_ref.py on its
inputs (tests/test_locate_cpu.py asserts on the same arrays that the 'corr' bar is at most 1e-8 there), their edges (rows that do not
count, offset and sliced operands, both candidate mappings, chunking), the best rule and the candidate formula bit for bit, and the
search end to end on the hashed model: planted on the grid, planted between grid points with the trace checked level by level, gain and
offset invariance, chunking, batched observed rows, Model_nefnet2 and Solver.locate."""
import random

import numpy as np
import pytest
import torch

import conftest
import corr_ref
import locate_ref
from locate_ref import B, EPS, IDS, SHAPES, case, end_variants
from test_model_gpu import DEV, batch_t, hashed_model, hashed_model2, make_cfg

pytestmark = pytest.mark.gpu
INF = float("inf")
MSE_REL = 1e-11          # the worst-case fp64 summation bound is n 2^-53: 4.5e-12 at n = 40000


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rois(ends):
    return None if ends is None else corr_ref.rois_of(ends).to(DEV)


def _offset(t):
    """The same values one float off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


_WORST = {"corr": 0.0, "mse": 0.0, "metrics": 0.0}


# ------------------------------------------------------------------------------------------------ 1. nef_locate_score
@pytest.mark.parametrize("R,A,L", SHAPES, ids=IDS)
def test_scores_against_the_restatement(R, A, L):
    """Both modes, both candidate mappings, every row-end variant: 'mse' within 1e-11 relative, 'corr' within the per-row bound
    3 delta / min(vx + eps, vy + eps) of the restatement (at most 1e-8: tests/test_locate_cpu.py), rows that do not count +inf; the
    'corr' score is 1 - r of ops.view_corr_metrics on obs expanded over the candidates within the same bound; a grouped call gives the
    bits of the all-pairs call (a row's score depends on that row alone).
    Worst measured on MI355X over all cases: the 'corr' error at 3.89e-3 of its bound, the metrics route at 2.04e-3 of it, 'mse' 7.56e-15
    relative (the `locate kernels:` line of the run's parity facts reports this run's numbers again)."""
    from electrocardio_panorama_amd import ops
    pred, obs = case(R, A, L)
    pd, od = g(pred), g(obs)
    G = A // R
    for ends in end_variants(L):
        n = locate_ref.row_ends(None if ends is None else corr_ref.rois_of(ends), B, L)
        rois = _rois(ends)
        for mode in ("mse", "corr"):
            want, bound = locate_ref.scores(pred, obs, n, mode, with_bound=True)
            got_d = ops.locate_score(pd, od, rois, mode, EPS)
            got = got_d.cpu().numpy()
            assert got.shape == (B, R, A) and got.dtype == np.float64
            assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isnan(got).any(), (ends, mode)
            assert np.isinf(want).all(axis=(1, 2)).tolist() == [v < (1 if mode == "mse" else 2) for v in n]
            fin = np.isfinite(want)
            if fin.any():
                err = np.abs(got[fin] - want[fin])
                if mode == "mse":
                    rel = float((err / want[fin]).max())
                    _WORST["mse"] = max(_WORST["mse"], rel)
                    print(f"R={R} A={A} L={L} ends={ends} mse: worst relative {rel:.2e}")
                    assert rel <= MSE_REL, (ends, rel)
                else:
                    ratio = float((err / bound[fin]).max())
                    _WORST["corr"] = max(_WORST["corr"], ratio)
                    print(f"R={R} A={A} L={L} ends={ends} corr: worst error / bound {ratio:.2e} (largest bound {bound[fin].max():.2e})")
                    assert ratio <= 1.0, (ends, ratio)
                    # the same number by the metrics kernel: obs row r expanded over the candidates
                    for r in range(R):
                        mom, cnt = ops.view_corr_metrics(pd, od[:, r:r + 1].expand(B, A, L).contiguous(), rois)
                        mom, cnt = mom.cpu().numpy(), cnt.cpu().numpy()
                        assert cnt[:, 0].tolist() == n
                        with np.errstate(invalid="ignore", divide="ignore"):
                            via = 1.0 - (mom[..., 2] + EPS) / np.sqrt((mom[..., 0] + EPS) * (mom[..., 1] + EPS))
                        f = fin[:, r]
                        ratio = float((np.abs(got[:, r][f] - via[f]) / bound[:, r][f]).max())
                        _WORST["metrics"] = max(_WORST["metrics"], ratio)
                        assert ratio <= 1.0, (ends, r, ratio)
            if G >= 1:        # candidate a against row a // G: the scores of the all-pairs call, bit for bit
                grouped = ops.locate_score(pd[:, :R * G], od, rois, mode, EPS, group=G)
                assert grouped.shape == (B, R, G)
                pick = torch.stack([got_d[:, r, r * G:(r + 1) * G] for r in range(R)], dim=1)
                assert torch.equal(grouped, pick), (ends, mode)
                wg = locate_ref.scores(pred[:, :R * G], obs, n, mode, group=G)
                assert np.array_equal(np.isinf(grouped.cpu().numpy()), np.isinf(wg))
    conftest.REPORT[:] = [ln for ln in conftest.REPORT if not ln.startswith("locate kernels:")]
    conftest.report(f"locate kernels: worst 'corr' error / bound {_WORST['corr']:.2e}, via view_corr_metrics {_WORST['metrics']:.2e}, "
                    f"'mse' relative {_WORST['mse']:.2e} (bar {MSE_REL:g})")


@pytest.mark.parametrize("L", [1, 2, 7, 64, 257, 1000, 1024, 1025, 5000])
def test_identical_rows_score_exactly_zero(L):
    from electrocardio_panorama_amd import ops
    _, obs = case(3, 5, 5000)
    od = g(obs[:, :, :L])
    for mode, least in (("mse", 1), ("corr", 2)):
        for ends in (None, [L, max(L - 1, 0)]):
            s = ops.locate_score(od, od, _rois(ends), mode, EPS, group=1).cpu().numpy()
            n = [L, L] if ends is None else ends
            for b in range(B):
                assert (s[b] == (0.0 if n[b] >= least else INF)).all(), (mode, ends, s[b])
            s = ops.locate_score(_offset(od), od, _rois(ends), mode, EPS, group=1).cpu().numpy()      # one aligned, one not
            for b in range(B):
                assert (s[b] == (0.0 if n[b] >= least else INF)).all(), (mode, ends, s[b])


@pytest.mark.parametrize("L", [7, 257, 512, 5000])
@pytest.mark.parametrize("mode", ["mse", "corr"])
def test_chunks_slices_and_offsets_give_identical_bits(L, mode):
    """A tensor scored at once, in chunks of 1 and 3 angles (slices of the larger pred, columns of the larger scores), from copies one float
    off a 16-byte boundary, and into a column window of a wider table: the same bits."""
    from electrocardio_panorama_amd import ops
    R, A = 3, 26
    pred, obs = case(R, A, L)
    pd, od = g(pred), g(obs)
    rois = _rois([L - 1, L])
    full = ops.locate_score(pd, od, rois, mode, EPS)
    for c in (1, 3):
        out = torch.full((B, R, A), -7.0, device=DEV, dtype=torch.float64)
        for a0 in range(0, A, c):
            part = pd[:, a0:a0 + c]
            assert part.data_ptr() != pd.data_ptr() or a0 == 0
            ops.locate_score(part, od, rois, mode, EPS, out=out, col=a0)
        assert torch.equal(out, full), c
    for p2, o2 in ((_offset(pd), od), (pd, _offset(od)), (_offset(pd), _offset(od))):
        assert torch.equal(ops.locate_score(p2, o2, rois, mode, EPS), full)
    wide = torch.full((B, R, A + 9), -7.0, device=DEV, dtype=torch.float64)
    window = wide[:, :, 4:4 + A]
    assert ops.locate_score(pd, od, rois, mode, EPS, out=window) is window
    assert torch.equal(window, full) and bool((wide[:, :, :4] == -7.0).all()) and bool((wide[:, :, 4 + A:] == -7.0).all())
    big = g(np.concatenate([pred, pred[:, ::-1]], axis=1))                     # pred as the front half of a larger tensor
    assert torch.equal(ops.locate_score(big[:, :A], od, rois, mode, EPS), full)
    obs_big = g(np.concatenate([obs, obs], axis=1))
    assert torch.equal(ops.locate_score(pd, obs_big[:, R:], rois, mode, EPS), full)


def test_ops_reject_bad_arguments():
    from electrocardio_panorama_amd import ops
    pred, obs = case(3, 5, 64)
    pd, od = g(pred), g(obs)
    with pytest.raises(ValueError, match="score"):
        ops.locate_score(pd, od, None, "l1")
    with pytest.raises(ValueError, match="group"):
        ops.locate_score(pd, od, None, "mse", group=2)
    with pytest.raises(ValueError, match="obs"):
        ops.locate_score(pd, od[:, :, :32].contiguous(), None, "mse")
    with pytest.raises(ValueError, match="dense rows"):
        ops.locate_score(pd[:, :, ::2], od[:, :, ::2], None, "mse")
    with pytest.raises(ValueError, match="rois"):
        ops.locate_score(pd, od, torch.zeros(3, 7, 2, dtype=torch.int64, device=DEV), "mse")
    with pytest.raises(ValueError, match="out"):
        ops.locate_score(pd, od, None, "mse", out=torch.empty(B, 3, 4, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="cands"):
        ops.locate_best(torch.zeros(B, 3, 5, device=DEV, dtype=torch.float64), torch.zeros(4, 2, device=DEV))
    from electrocardio_panorama_amd._lib import NefLibraryError
    with pytest.raises(NefLibraryError, match="NEF_E_SHAPE"):
        ops.locate_score(pd, od, None, "corr", eps=0.0)


# ------------------------------------------------------------------------------------------------ 2. nef_locate_best, nef_locate_cands
def _same_best(got, want):
    bs, bt, bi = (t.cpu().numpy() for t in got)
    assert np.array_equal(bs, want[0]), (bs, want[0])
    assert np.array_equal(bt, want[1], equal_nan=True) and bt.dtype == np.float32, (bt, want[1])
    assert np.array_equal(bi, want[2]) and bi.dtype == np.int64, (bi, want[2])


def _planted_scores(R, A, L=64):
    """The device's own scores with a tie at the minimum, NaN and inf columns and a pair without a finite score."""
    from electrocardio_panorama_amd import ops
    pred, obs = case(R, A, L)
    s = ops.locate_score(g(pred), g(obs), None, "corr", EPS)
    lo = s.min(dim=2).values
    s[:, :, 20] = lo                       # a tie behind (or at) the minimum: the earliest column keeps it
    s[0, 0, 3] = lo[0, 0]                  # ... and one in front of it, in another lane
    s[:, :, 7] = float("nan")
    s[:, :, 11] = INF
    s[1, R - 1, :] = INF                   # no finite score at all
    s[1, R - 1, 5] = float("nan")
    return s


def test_best_rule_on_the_devices_own_scores():
    from electrocardio_panorama_amd import ops
    R, A = 3, 26
    s = _planted_scores(R, A)
    sn = s.cpu().numpy()
    cands = np.random.default_rng(5).random((A, 2), dtype=np.float32)
    want = locate_ref.best_table(sn, cands)
    assert want[2][1, R - 1] == -1 and want[2][0, 0] <= 3 and (want[2][:, :] <= 20).all()
    got = ops.locate_best(s, g(cands))
    _same_best(got, want)
    # merging across three calls: column slices of the table, index_base = the slice's first column; in place
    best = None
    for a0, a1 in ((0, 9), (9, 18), (18, 26)):
        out = ops.locate_best(s[:, :, a0:a1], g(cands[a0:a1]), best, index_base=a0)
        assert best is None or all(o is b_ for o, b_ in zip(out, best))
        best = out
    _same_best(best, want)
    # ... and in another order of the slices the tie rule is the order of the calls: the restatement says the same
    best, run = None, None
    for a0, a1 in ((18, 26), (0, 9), (9, 18)):
        best = ops.locate_best(s[:, :, a0:a1], g(cands[a0:a1]), best, index_base=a0)
        run = locate_ref.best_table(sn[:, :, a0:a1], cands[a0:a1], run, index_base=a0)
    _same_best(best, run)
    assert run[2][1, 0] in (18, 19, 20)                     # the slice called first keeps the tie
    # more candidates than lanes, the minimum planted in several lanes and passes
    wide = torch.rand(B, 2, 300, device=DEV, dtype=torch.float64) + 1.0
    for col in (299, 130, 66, 257):
        wide[0, 0, col] = 0.5
    wide[1, 1, 64] = wide[1, 1, 0] = 0.25
    c3 = np.random.default_rng(6).random((300, 2), dtype=np.float32)
    got = ops.locate_best(wide, g(c3))
    _same_best(got, locate_ref.best_table(wide.cpu().numpy(), c3))
    assert got[2].tolist()[0][0] == 66 and got[2].tolist()[1][1] == 0


def test_best_rule_with_per_pair_candidates():
    from electrocardio_panorama_amd import ops
    R, G = 3, 25
    rng = np.random.default_rng(9)
    s0 = _planted_scores(R, 26)
    c0 = rng.random((26, 2), dtype=np.float32)
    best = ops.locate_best(s0, g(c0))
    run = locate_ref.best_table(s0.cpu().numpy(), c0)
    for level in range(3):
        sc = torch.from_numpy(rng.random((B, R, G)) * (2.0 - 0.6 * level)).to(DEV)
        sc[:, :, 4] = float("nan")
        sc[0, 1, :] = INF                                   # a level where nothing is finite: the running best stays
        sc[1, 0, 9] = sc[1, 0, 17] = -1.0                   # a tie below everything: column 9's candidate
        cands = rng.random((B, R * G, 2), dtype=np.float32)
        index_before = best[2].clone()
        out = ops.locate_best(sc, g(cands), best, keep_index=True)
        assert all(o is b_ for o, b_ in zip(out, best)) and torch.equal(best[2], index_before)
        run = locate_ref.best_table(sc.cpu().numpy(), cands, run, keep_index=True)
        _same_best(best, run)
        if level == 0:                                      # (later levels tie with it at -1.0: not strictly lower, it stays)
            first = cands[1, 0 * G + 9].copy()
        assert np.array_equal(best[1][1, 0].cpu().numpy(), first) and float(best[0][1, 0]) == -1.0
    assert int(best[2][1, R - 1]) == -1 and float(best[0][1, R - 1]) == INF and bool(torch.isnan(best[1][1, R - 1]).all())


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_candidates_match_the_fp32_formula_bit_for_bit(radius):
    from electrocardio_panorama_amd import locate, ops
    grid = locate.Grid()
    rng = np.random.default_rng(radius)
    bt = (rng.random((B, 3, 2), dtype=np.float32) * np.float32(3.0) - np.float32(1.5)).astype(np.float32)
    bi = rng.integers(0, 171, size=(B, 3))
    bi[0, 1] = bi[1, 2] = -1                                # placeholder rows
    bt[0, 1] = bt[1, 2] = np.nan
    ph = tuple(grid.thetas()[0])
    for s1, s2 in locate.level_steps(grid, 4) + [(np.float32(0.0), np.float32(0.1))]:
        got = ops.locate_cands(g(bt), g(bi), s1, s2, radius, ph).cpu().numpy()
        want = locate_ref.level_cands(bt, bi, s1, s2, radius, ph)
        assert got.dtype == np.float32 and got.shape == want.shape == (B, 3 * (2 * radius + 1) ** 2, 2)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.isfinite(got).all()
        mid = (2 * radius + 1) ** 2 // 2
        assert np.array_equal(got[0, mid], bt[0, 0]) and np.array_equal(got[0, (2 * radius + 1) ** 2 + mid], np.asarray(ph))


# ------------------------------------------------------------------------------------------------ 3. end to end
GRID_N = (4, 6)
# Screening for (a)'s precondition (the runner-up's score at the planted grid points is at least 1e-6), measured on MI355X from views the
# screening decoded, in fp64 on the CPU.  Seeds 31 .. 38 of batch_t(2, 3, 512, seed), 4 x 6 grids over four ranges, PLANT below:
#   LEAD_THETA's span (the default range): 'mse' on Model_nefnet has its runner-up at 2.6e-8 .. 6.2e-8 on EVERY seed, fp32 and fp16 -- the
#     hashed (untrained) weights barely turn the view with the angle, 1e-4 rms over a 40-degree step; 'corr' is at 9e-3 .. 3e-2.  No seed
#     can mend a factor of 20, so the range was screened too (the Angular Encoding holds the raw angle: any range is a valid query);
#   [0, 2 pi] x [-pi, pi]: 'mse' 1.2e-7 .. 2.9e-7, fails;  [-pi, 3 pi] x [-3 pi, 3 pi]: 8.6e-7 .. 1.5e-6, holds on some seeds only;
#   [-4 pi, 6 pi] x [-6 pi, 6 pi]: holds on every seed screened, both modes, both dtypes, both model classes.  Seed 31, the first:
#     Model_nefnet 'mse' 2.08e-6 / 2.77e-6 (fp32 and fp16), 'corr' 9.4e-2 / 1.1e-1; Model_nefnet2 'mse' 2.2e-4 / 2.6e-5, 'corr' 1.7e-2 / 5.8e-2.
# The tests assert the precondition again on the views they decode.
GRID_RANGE = (-4 * np.pi, 6 * np.pi, -6 * np.pi, 6 * np.pi)
_E2E_SEED = 31
PLANT = (7, 16)          # grid indices of the views planted for sample 0 and 1


def _grid():
    from electrocardio_panorama_amd import locate
    return locate.Grid(*GRID_N, *GRID_RANGE)


def _decode(m, b, thetas):
    """Views [B, Q, L] of the batch at per-sample angles [B, Q, 2], decoded by the test itself."""
    from electrocardio_panorama_amd import engine, ops
    z1, z2 = m(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="gen")
    if type(m).__name__ == "Model_nefnet":
        return m.gen_ecg(z1, z2, thetas, b["rois"])
    with torch.no_grad(), ops.amax_scope((m._nef_scope, False)):                  # Model_nefnet2: phase 'gen' returns the two lead means
        return engine.sweep(m._params_by_name(), m._buffers_by_name(), torch.cat([z1, z2], dim=1).contiguous(), thetas.contiguous(), False, 8,
                            m._half_sweep())


def _grid_views(m, b):
    th = g(_grid().thetas())
    return th, _decode(m, b, th.unsqueeze(0).expand(b["data"].shape[0], -1, -1).contiguous())


def _ends(b):
    return locate_ref.row_ends(b["rois"].cpu(), b["rois"].shape[0], b["data"].shape[-1])


def _planted_on_the_grid(m, mode, dtype):
    m.panorama_dtype = dtype
    b = batch_t(2, 3, 512, _E2E_SEED)
    th, views = _grid_views(m, b)
    observed = torch.stack([views[i, k] for i, k in enumerate(PLANT)]).contiguous()
    # the precondition, in fp64 on the CPU from the views decoded here: the runner-up is at least 1e-6 away
    ref = locate_ref.scores(views.cpu().numpy(), observed.unsqueeze(1).cpu().numpy(), _ends(b), mode)[:, 0]
    for i, k in enumerate(PLANT):
        assert ref[i, k] == 0.0
        runner = float(np.delete(ref[i], k).min())
        print(f"{type(m).__name__} {dtype} {mode} sample {i}: runner-up {runner:.3e}")
        assert runner >= 1e-6, (i, runner)
    res = m.locate(b["data"], b["input_theta"], b["rois"], observed, grid=_grid(), score=mode, levels=0, return_scores=True)
    assert res.index.tolist() == list(PLANT) and res.index.dtype == torch.int64
    assert torch.equal(res.theta, th[list(PLANT)]) and torch.equal(res.theta0, res.theta)
    assert float(res.score.max()) <= 1e-9 and torch.equal(res.score, res.score0)
    assert res.scores.shape == (2, GRID_N[0] * GRID_N[1]) and res.trace is None
    assert float((res.scores.cpu() - torch.from_numpy(ref)).abs().max()) <= 1e-9
    assert not m.training


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("mode", ["mse", "corr"])
def test_a_view_planted_on_the_grid_is_found(mode, dtype):
    _planted_on_the_grid(hashed_model(3).eval(), mode, dtype)


def test_model_nefnet2_finds_a_planted_view():
    _planted_on_the_grid(hashed_model2(3).eval(), "mse", "fp32")


@pytest.mark.parametrize("mode", ["mse", "corr"])
def test_planted_between_grid_points_the_trace_is_the_search(mode):
    """R = 2, levels = 3: every level's candidates are the formula from the previous best, every level's winner is the arg-best of the
    trace's own scores under the tie rule, the running best carries over (score <= score0), theta stays within (1 - 2^-levels) 2 d of
    theta0 on each axis (+ 4 x 2^-24 x max |theta|: the three rounded fp32 adds and the fp32 rounding of d), and the trace's scores are those of views the
    test decodes itself at the traced candidates (1e-4 relative: each candidate group met its own observed row).  The distance to the
    planted angle is reported, not asserted: an untrained model's score landscape need not be unimodal."""
    from electrocardio_panorama_amd import locate
    m = hashed_model(3).eval()
    b = batch_t(2, 3, 512, _E2E_SEED)
    grid, levels, radius = _grid(), 3, 2
    d1, d2 = grid.steps
    th = grid.thetas()
    planted = np.stack([[th[7] + np.float32([0.37 * d1, -0.21 * d2]), th[14] + np.float32([-0.45 * d1, 0.3 * d2])],
                        [th[16] + np.float32([0.12 * d1, 0.41 * d2]), th[3] + np.float32([0.33 * d1, 0.25 * d2])]]).astype(np.float32)
    observed = _decode(m, b, g(planted)).contiguous()                                   # [B, 2, L]
    res = m.locate(b["data"], b["input_theta"], b["rois"], observed, grid=grid, score=mode, levels=levels, radius=radius,
                   return_scores=True, return_trace=True)
    ends, obs_np = _ends(b), observed.cpu().numpy()
    G = (2 * radius + 1) ** 2
    # level 0: the arg-best of the returned table
    run = locate_ref.best_table(res.scores.cpu().numpy(), th)
    _same_best((res.score0, res.theta0, res.index), run)
    assert len(res.trace) == levels and (run[2] >= 0).all()
    for lv, (s1, s2) in zip(res.trace, locate.level_steps(grid, levels)):
        cands = lv["cands"].cpu().numpy()
        want = locate_ref.level_cands(run[1], run[2], s1, s2, radius, tuple(th[0]))
        assert np.array_equal(cands.view(np.uint32), want.view(np.uint32))
        sc = lv["scores"].cpu().numpy()
        assert sc.shape == (2, 2, G)
        run = locate_ref.best_table(sc, cands, run, keep_index=True)
        _same_best((lv["score"], lv["theta"], res.index), run)
        # the scores are those of the views at these candidates against the pair's own observed row
        mine = locate_ref.scores(_decode(m, b, lv["cands"]).cpu().numpy(), obs_np, ends, mode, group=G)
        assert float((np.abs(sc - mine) / np.abs(mine)).max()) <= 1e-4
    _same_best((res.score, res.theta, res.index), run)
    assert bool((res.score <= res.score0).all())
    reach = (1.0 - 2.0 ** -levels) * 2.0 * np.array([d1, d2])
    moved = np.abs(res.theta.cpu().numpy().astype(np.float64) - res.theta0.cpu().numpy().astype(np.float64))
    top = max(float(np.abs(th).max()), float(res.theta.abs().max()))
    assert (moved <= reach + 4 * 2.0 ** -24 * top).all(), (moved, reach)
    off = np.degrees(np.abs(res.theta.cpu().numpy() - planted)).reshape(-1, 2).max(axis=0)
    off0 = np.degrees(np.abs(res.theta0.cpu().numpy() - planted)).reshape(-1, 2).max(axis=0)
    conftest.report(f"locate {mode}, planted between grid points (hashed weights, 4 x 6 grid, 3 levels): largest distance to the planted "
                    f"angle {off[0]:.2f} / {off[1]:.2f} deg (level 0: {off0[0]:.2f} / {off0[1]:.2f} deg)")


def test_gain_offset_chunking_and_batched_rows():
    """(c) 'corr' finds the same index for 0.5 * observed + 0.2; (d) chunk = 5 and one chunk give the same index and theta; (e) a 2-D
    observed is row 0 of the [B, 1, L] call, and an R = 3 call equals three R = 1 calls in index."""
    m = hashed_model(3).eval()
    b = batch_t(2, 3, 512, _E2E_SEED)
    grid = _grid()
    _, views = _grid_views(m, b)
    obs3 = torch.stack([views[0, [7, 2, 21]], views[1, [16, 9, 0]]]).contiguous()       # [B, 3, L]
    call = lambda o, **kw: m.locate(b["data"], b["input_theta"], b["rois"], o, grid=grid, **kw)      # noqa: E731
    three = call(obs3)
    assert three.index.tolist() == [[7, 2, 21], [16, 9, 0]] and three.theta.shape == (2, 3, 2) and three.score.shape == (2, 3)
    moved = call((0.5 * obs3 + 0.2).contiguous())
    assert torch.equal(moved.index, three.index)                                         # (c)
    chunked = call(obs3, chunk=5)
    assert torch.equal(chunked.index, three.index) and torch.equal(chunked.theta, three.theta)      # (d)
    for r in range(3):                                                                   # (e)
        one = call(obs3[:, r:r + 1].contiguous())
        flat = call(obs3[:, r].contiguous())
        assert one.index.shape == (2, 1) and flat.index.shape == (2,) and flat.theta.shape == (2, 2)
        assert torch.equal(one.index[:, 0], three.index[:, r])
        for a, c in zip(flat[:5], one[:5]):
            assert torch.equal(a, c[:, 0])
    m.train()
    call(obs3[:, 0].contiguous(), levels=0)
    assert m.training                                                                    # the mode it was in


def test_solver_locate_on_a_synthetic_batch(capsys):
    """(g) One synthetic batch: finite numbers under every name in last_locate, the model's training flag restored, Python's random
    stream and the forward counter untouched, psnr_gen bit-identical with the key on and off, and no locate launch with it off."""
    from electrocardio_panorama_amd import ops, synth
    from electrocardio_panorama_amd.solver import Solver
    from oracle import hashweights as hw
    V, Bn, L, Q = 3, 2, 512, 6
    test = [dict(synth.make_batch(Bn, V, L, seed=70, Q=Q))]
    runs = {}
    for name, keys in (("off", {}), ("on", dict(locate_eval=True, locate_grid=[4, 6], locate_levels=2))):
        cfg = make_cfg(V)
        cfg.DATA["synthetic"], cfg["seed"] = True, 7
        cfg.SOLVER.update(keys)
        sol = Solver(cfg, use_tensorboardx=False)
        sol.model.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
        assert sol.locate_eval is (name == "on") and sol.last_locate is None
        random.seed(101)
        with torch.no_grad():
            before = sol.run_one_epoch(test, "test", collect_views=False)[4]
            if name == "on":
                sol.model.train()
                state, calls = random.getstate(), sol.model._drop_calls
                out = sol.locate(test)
                assert sol.model.training and random.getstate() == state and sol.model._drop_calls == calls
                assert out is sol.last_locate
                print(sol._locate_message())
            after = sol.run_one_epoch(test, "test", collect_views=False)[4]
        runs[name] = (before, after, sol.last_locate)
    assert runs["off"][2] is None
    assert runs["off"][0] == runs["on"][0] and runs["off"][1] == runs["on"][1]           # psnr / ssim: the same bits, before and behind
    got = runs["on"][2]
    names = [f"locate_{k}_{s}" for s in ("gen", "reg") for k in ("err1", "err1_med", "err2", "err2_med", "hit")]
    assert sorted(got) == sorted(names)
    assert all(np.isfinite(v) for v in got.values()), got
    assert all(0.0 <= got[f"locate_hit_{s}"] <= 1.0 for s in ("gen", "reg")) and all(v >= 0.0 for v in got.values())
    text = capsys.readouterr().out
    assert "locate_err1_gen:" in text and "locate_hit_reg:" in text
    conftest.report("Solver.locate (hashed weights, one synthetic batch, 4 x 6 grid, 2 levels): " + ", ".join(f"{k} {v:.3g}" for k, v in got.items()))
