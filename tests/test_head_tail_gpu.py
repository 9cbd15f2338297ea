"""The thin ops at the two ends of the network -- the output conv (csrc/elementwise.hip), the loss, the angular encoding
and its linear layer (csrc/convt_theta.hip), the channel scale, roi_align (csrc/roi.hip) and the window crop / scatter --
against the fp64 restatements of tests/head_tail_ref.py, every element, at the smallest shapes that reach each branch.

Bars.  u = 2^-24.  Next to every norm of the project (1e-6 forward, GRAD_TOL / 1e-5 gradients, FWD_TOL for the linear
layer) stands a bound for EVERY element, stated against the sum of magnitudes the rounding errors scale with (head_tail_ref
returns it next to each value).  Each constant is derived below from the kernel's own arithmetic;
tests/test_head_tail_ref_cpu.py runs an fp32 restatement of every one of them, in the kernel's order of operations, on
the CPU and asserts that it stays inside the same bound: no constant was fitted to a kernel's output.  The comparison
(head_tail_ref.frac) fails on a NaN or an infinity, not only on a finite value outside its bound.
  A  outconv_fwd: |d| <= (3C+2) u S/12 + 6u, S = sum|w_k||act_k| + |bias|: the 3C-fma chain and the bias add through the
     slope of sigmoid(z/3) (at most 1/12), then expf, the add and the division.
     outconv_bwd_data: |d| <= 8u sum_k|w_k||go_k|: go = gout*(o*(1-o))/3 is four roundings (the relative error on go), the
     three-tap sum three more, one spare.
     outconv_bwd_weight: |d| <= K u sum|go||act| for each of the 3C values, K u sum|go| for the bias gradient, with
     K = 12 + 16 * ceil(units / 1024), units = N * ceil(L / 1024): go carries 4u, a prologue's fma 1u, a lane chains
     16 fmas per (sample, tile) unit and a block takes ceil(units / 1024) units (gamma_m <= m u), the wave sum is a
     6-level tree (6u), the block partials are summed in fp64 and rounded once (1u).  K = 28 where one block takes one
     unit, 44 for the two unit-loop shapes.
  B  loss values: 4u relative per term; gradients 6u relative per element; exactly 0.0 wherever the reference is 0
     (masked terms, planted ties o == tgt, o == pp, o == pl).
  C  theta_encode: 2e-6 absolute (the project's bar); theta_mlp_fwd: 14u (sum|e_k W_k| + |bias|) + 2e-6 sum|W_k| (12 fmas,
     the bias add, one spare; the second term carries the encoding's bar through the layer); theta_mlp_bwd:
     gW within 2u sum|g e_k| + 2e-6 sum|g| (one rounding per product, fp64 sums, one final rounding); gb, which the
     encoding never enters, within 2u sum|g|.
  D  chscale: y and gx one rounding (u relative), gx exactly 0 under the relu_x mask, gs within (T/64 + 8) u sum|gy x|
     (a lane chains ceil(T/64) fmas, the wave tree adds 6).
  E  roi_align_fwd: 4u (|z0 w0| + |z1 w1|) wx; roi_align_bwd: (112/64 + 8) u w_row sum|gout wx| on the two middle rows,
     exactly 0 elsewhere; the windowed forms equal the full ones bit for bit.
  F  window_crop / window_scatter: exact.

Decision ties.  The prologue cases decide a ReLU on fmaf(x, a, b) > 0 where the reference decides on x*a + b in fp64.
As in test_bn_gpu.py every such case first ASSERTS that no decision of its inputs is closer to a tie than
MARGIN = 2^-16 of |x*a| + |b| and then compares everything; nothing is masked out.  SEEDS holds a seed per prologue shape
(searched on the CPU: `python tests/test_head_tail_gpu.py`); test_head_tail_ref_cpu.py asserts the screen for the
whole table without a GPU.  chscale's relu_x decides on the input x itself (x > 0): no arithmetic, no tie; its cases plant
+0.0, -0.0 and negative values instead, and the CPU file asserts that they are there.

Wrong-on-purpose edits of the kernels tried against this file on the MI355X (one build per edit, only the tests named
run, none committed; every edit changes arithmetic or skips work, none moves an index or a guard).  Edits 1 to 4 skip
work only at sizes the per-op tests of tests/test_ops_gpu.py never reach: its outconv, loss and theta tests were run
against each of the four and all passed, so that file alone catches none of them.
   1  outconv_bwd_weight_partial leaves its unit loop after the first unit -> test_outconv_bwd_weight (1030,3,4), (520,3,1028)
   2  `b += 512` in outconv_bwd_weight_final -> test_outconv_bwd_weight (1030,3,4), (520,3,1028)
   3  loss_partial's stride doubled -> test_loss n = 65793, l1 and l2 (the value is off by 16000 bounds)
   4  `n += 512` in theta_mlp_bwd_kernel -> test_theta_mlp_bwd N = 257 and 700, both O
   5  `hl` false in outconv_fwd_kernel<true> -> test_outconv_fwd_bwd_data at every L % 4 == 0 with L >= 12, both forms
   6  the `if (!hr) v[5] = 0.f` line dropped -> test_outconv_fwd_bwd_data at the four prologue shapes with L % 4 == 0
   7  `xp` forced 0 in the scalar forward, tried in both readings -- `float xp = 0.f` where it is loaded (a prologue then
      turns it into relu(b)), and the right tap multiplied by 0 -- -> either way test_outconv_fwd_bwd_data at every
      L % 4 != 0 with L >= 2, the prologue shape (2,3,5,1025) included
   8  taps 0 and 2 swapped in outconv_bwd_data_kernel -> test_outconv_fwd_bwd_data at every shape with L >= 2
   9  sgnf(0) returning 1 -> test_loss at every (reg, n) but (l2, 1), whose only planted tie is o == tgt under 2(o - tgt)
  10  `ph - th` in encode12 -> test_theta_encode, every test_theta_mlp_fwd and test_theta_mlp_bwd case
  11  `b * C` for `b * s_bs` in chscale_bwd_kernel -> test_chscale, the twelve s_column_block cases
  12  `!(xv >= 0.f)` for the relu_x mask -> test_chscale, the twelve relu_x cases
  13  `e += 128` in roi_align_bwd_kernel -> test_roi_align_golden and test_roi_align_synth, every case
  14  `t > t0` in window_scatter_kernel -> test_window_crop_scatter, both shapes
"""
import numpy as np
import pytest
import torch

import head_tail_ref as R
from util import FWD_TOL, GRAD_TOL, maxabs, rel, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
U, MARGIN = R.U, R.MARGIN

# ------------------------------------------------------------------------------------------------ shapes
OC_PLAIN = [(2, 3, 1), (2, 3, 2), (2, 3, 3), (2, 3, 4), (2, 3, 5), (3, 64, 12), (2, 5, 257), (3, 64, 260), (2, 3, 1025),
            (3, 17, 1028), (1, 3, 2052)]                                        # (N, C, L)
OC_PRO = [(3, 2, 64, 12), (3, 2, 64, 260), (3, 2, 17, 1028), (3, 1, 3, 2052), (2, 3, 5, 1025)]      # (P, Bp, C, L)
OC_UNITS = [(1030, 3, 4), (520, 3, 1028)]                                       # more units than OC_BLOCKS = 1024 blocks
# (P, Bp, C, L) -> seed whose prologue decisions clear the tie screen
SEEDS = {(3, 2, 64, 12): 2000, (3, 2, 64, 260): 2001, (3, 2, 17, 1028): 2001, (3, 1, 3, 2052): 2000, (2, 3, 5, 1025): 2000}

LOSS_N = [1, 255, 2000, 65536 + 257]
LOSS_FACTORS = R.LOSS_FACTORS
CHSCALE_SHAPES = [(3, 50, 77), (2, 5, 1), (2, 5, 63), (2, 5, 64), (2, 5, 65), (40, 130, 3)]
ROI_L = R.ROI_L

WORST = {}      # family -> (worst error / bound, where): one parity-facts line per family when the module is done


def ops():
    from electrocardio_panorama_amd import ops as o
    return o


def g(t):
    return torch.as_tensor(t).float().to(DEV).contiguous()


def elem(family, where, got, ref, bound):
    """Assert the per-element bound and keep the family's worst fraction of it."""
    f = R.frac(got, ref, bound)
    print(f"{family} {where}: worst error / bound {f:.3f}")
    if f > WORST.get(family, (-1.0, ""))[0]:
        WORST[family] = (f, where)
    assert f <= 1.0, (family, where, f)
    return f


@pytest.fixture(scope="module", autouse=True)
def _family_lines():
    yield
    import conftest
    names = dict(A="output conv", B="loss", C="theta", D="channel scale", E="roi_align", F="window crop / scatter")
    for k in sorted(WORST):
        f, where = WORST[k]
        conftest.report(f"head/tail {k} ({names[k]}): worst element error / bound {f:.3f} at {where}")


# ------------------------------------------------------------------------------------------------ A. output conv
def oc_case(shape):
    """The case's seeded inputs (head_tail_ref.oc_case): the screened seed of SEEDS for a prologue shape."""
    return R.oc_case(shape, SEEDS[shape] if len(shape) == 4 else R.OC_PLAIN_SEED)



def oc_screen(c):
    """The tie screen of a prologue case: asserted, never skipped; nothing is excluded from what follows."""
    if c["pro"] is None:
        return None
    m = R.pro_margin(c["x"], c["pro"])
    assert m >= MARGIN, f"seed {c['seed']}: closest prologue decision at {m:.2e} < 2^-16"
    return m


def dev_pro(c):
    return None if c["pro"] is None else (g(c["pro"][0]), g(c["pro"][1]), c["pro"][2])


@pytest.mark.parametrize("shape", OC_PLAIN + OC_PRO, ids=str)
def test_outconv_fwd_bwd_data(shape):
    """outconv_fwd_kernel<true> (L % 4 == 0; L = 1028, 2052: a second and third 1024-column tile) and <false> (L = 257,
    1025: the second and fifth 256-column tile), C = 3 .. 64, with and without the prologue; outconv_bwd_data_kernel on the
    same shapes (256-column tiles at every L)."""
    o = ops()
    c = oc_case(shape)
    oc_screen(c)
    C = c["C"]
    out = o.outconv_fwd(g(c["x"]), g(c["w"]), g(c["b"]), pro=dev_pro(c))
    assert out.shape == c["ref"].shape and rel(out, c["ref"]) < 1e-6
    S = R.outconv_S(c["x"], c["w"], c["b"], c["pro"])
    elem("A", f"outconv_fwd {shape}", out, c["ref"], (3 * C + 2) * U * S / 12 + 6 * U)
    gx = o.outconv_bwd_data(g(c["gy"]), g(c["out"]), g(c["w"]), C)
    gref, gmag = R.outconv_bwd_data(c["gy"], c["out"], c["w"])
    assert gx.shape == gref.shape and rel(gx, gref) < GRAD_TOL
    elem("A", f"outconv_bwd_data {shape}", gx, gref, 8 * U * gmag)


@pytest.mark.parametrize("shape", OC_PLAIN + OC_PRO + OC_UNITS, ids=str)
def test_outconv_bwd_weight(shape):
    """outconv_bwd_weight_partial (both branches, the 1024-column tile seam and its halo, C % 16 != 0, the unit loop at
    (1030,3,4) and (520,3,1028)) + outconv_bwd_weight_final (nblk = 1024 > 256 there), with and without the prologue."""
    o = ops()
    c = oc_case(shape)
    oc_screen(c)
    gw, gb = o.outconv_bwd_weight(g(c["gy"]), g(c["out"]), g(c["x"]), pro=dev_pro(c))
    rw, rb, aw, ab = R.outconv_bwd_weight(c["gy"], c["out"], c["x"], c["pro"])
    assert gw.shape == rw.shape and rel(gw, rw) < 1e-5 and rel(gb, rb) < 1e-5
    K = R.oc_weight_K(c["N"], c["L"])
    elem("A", f"outconv_bwd_weight gw {shape}", gw, rw, K * U * aw)
    elem("A", f"outconv_bwd_weight gb {shape}", gb, rb, K * U * ab)


# ------------------------------------------------------------------------------------------------ B. loss
PLANT = R.PLANT


def rel_or_zero(family, where, got, ref, k):
    """Exactly 0.0 wherever the reference is 0, within k u relative elsewhere."""
    got, ref = R.d(got).reshape(-1), R.d(ref).reshape(-1)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), f"{where}: a value is not finite"
    zero = ref == 0
    assert bool((got[zero] == 0).all()), f"{where}: {int((got[zero] != 0).sum())} values are not exactly 0 where the reference is"
    if bool((~zero).any()):
        elem(family, where, got[~zero], ref[~zero], k * U * ref[~zero].abs())


@pytest.mark.parametrize("n", LOSS_N)
@pytest.mark.parametrize("reg_l2", [False, True], ids=["l1", "l2"])
def test_loss(reg_l2, n):
    """loss_partial + loss_final and loss_bwd_kernel: every mask 1..7, with and without the noise row, gscale None, [1.0]
    and [0.37]; n = 65793 takes the grid-stride loop of loss_partial (256 blocks of 256); planted exact ties."""
    o = ops()
    c = R.loss_case(n)
    dv = {k: g(c[k]) for k in ("pp", "pl", "tgt", "noise")}
    for noisy in (False, True):
        pred, noise = c["pred"][noisy], (c["noise"] if noisy else None)
        oo = R.loss_o(pred, noise)
        for i, other in zip(c["idx"], (c["tgt"], c["pp"], c["pl"])):
            assert len(i) == 0 or bool((oo[i] == R.d(other)[i]).all()), "a planted tie is not exact"
        pd, nd = g(pred), (dv["noise"] if noisy else None)
        for mask in range(1, 8):
            where = f"n={n} {'l2' if reg_l2 else 'l1'} mask={mask} noise={int(noisy)}"
            got = o.loss_fwd(pd, dv["pp"], dv["pl"], dv["tgt"], LOSS_FACTORS, reg_l2, mask, noise=nd)
            ref = R.loss(pred, c["pp"], c["pl"], c["tgt"], LOSS_FACTORS, reg_l2, mask, noise)
            rel_or_zero("B", f"loss_fwd {where}", got, ref, 4)
            for gsv in (None, 1.0, 0.37):
                gs = None if gsv is None else torch.tensor([gsv], dtype=torch.float32)
                gots = o.loss_bwd(pd, dv["pp"], dv["pl"], dv["tgt"], None if gs is None else g(gs), LOSS_FACTORS, reg_l2, mask, noise=nd)
                refs = R.loss_grads(pred, c["pp"], c["pl"], c["tgt"], gs, LOSS_FACTORS, reg_l2, mask, noise)
                for name, a, b in zip(("g_pred", "g_p", "g_l"), gots, refs):
                    assert a.shape == pred.shape
                    rel_or_zero("B", f"loss_bwd {name} {where} gscale={gsv}", a, b, 6)


# ------------------------------------------------------------------------------------------------ C. theta
def test_theta_encode(golden_dir):
    """theta_encode_kernel on the golden table and on the grid: 2e-6 absolute per element."""
    o = ops()
    z = np.load(f"{golden_dir}/theta_table.npz")
    enc = o.theta_encode(g(torch.from_numpy(z["theta"])))
    assert enc.shape == z["enc"].shape and maxabs(enc, z["enc"]) < 2e-6
    elem("C", "theta_encode golden", enc, R.theta_encode(z["theta"]), 2e-6)
    th = R.theta_grid()
    enc = o.theta_encode(g(th))
    assert enc.shape == (th.shape[0], 12)
    elem("C", f"theta_encode grid of {th.shape[0]}", enc, R.theta_encode(th), 2e-6)


@pytest.mark.parametrize("O", [5, 128, 256])
@pytest.mark.parametrize("N", [1, 18, 257, 300])
def test_theta_mlp_fwd(N, O):
    """theta_mlp_fwd_kernel: O = 256 is mlp2's width, O = 5 no multiple of 64."""
    o = ops()
    th, W, b = rnd(N, 2, seed=2400, scale=3.0), rnd(O, 12, seed=2401), rnd(O, seed=2402)
    y = o.theta_mlp_fwd(g(th), g(W), g(b))
    ref, A, Wabs = R.theta_mlp(th, W, b)
    assert y.shape == ref.shape and rel(y, ref) < FWD_TOL
    elem("C", f"theta_mlp_fwd N={N} O={O}", y, ref, 14 * U * A + 2e-6 * Wabs[None, :])


@pytest.mark.parametrize("O", [128, 5])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 700])
def test_theta_mlp_bwd(N, O):
    """theta_mlp_bwd_kernel: N > 256 takes the row loop (a thread sums rows n, n + 256, ...)."""
    o = ops()
    th, gy = rnd(N, 2, seed=2410, scale=3.0), rnd(N, O, seed=2411)
    gW, gb = o.theta_mlp_bwd(g(th), g(gy), O)
    rW, rb, AW, Ab = R.theta_mlp_grads(th, gy)
    assert gW.shape == rW.shape and gb.shape == rb.shape and rel(gW, rW) < GRAD_TOL and rel(gb, rb) < GRAD_TOL
    elem("C", f"theta_mlp_bwd gW N={N} O={O}", gW, rW, 2 * U * AW + 2e-6 * Ab[:, None])
    # gb is the fp64 sum of the fp32 g rounded once: the encoding never enters it, so its 2e-6 term is left out (sharper)
    elem("C", f"theta_mlp_bwd gb N={N} O={O}", gb, rb, 2 * U * Ab)


# ------------------------------------------------------------------------------------------------ D. channel scale
@pytest.mark.parametrize("relu_x", [False, True], ids=["plain", "relu_x"])
@pytest.mark.parametrize("strided", [False, True], ids=["s_contiguous", "s_column_block"])
@pytest.mark.parametrize("shape", CHSCALE_SHAPES, ids=str)
def test_chscale(shape, strided, relu_x):
    """chscale_fwd_kernel / chscale_bwd_kernel: T below, at and above one wave trip, rows > 4 * blocks at (40,130,3), `s`
    contiguous or a column block of a wider table (s_bs = 3C), relu_x on exact zeros of both signs."""
    o = ops()
    B, C, T = shape
    x, tab, gy = R.chscale_case(shape, relu_x)
    s = tab[:, C:2 * C]
    if strided:
        sd, s_bs = g(tab)[:, C:2 * C], 3 * C
        assert not sd.is_contiguous() or B == 1
    else:
        sd, s_bs = g(s), None
    where = f"{shape} {'s_bs=3C' if strided else 's_bs=C'} relu_x={int(relu_x)}"
    y, yref = o.chscale_fwd(g(x), sd, s_bs), R.chscale(x, s)
    assert rel(y, yref) < 1e-6
    elem("D", f"chscale_fwd {where}", y, yref, U * yref.abs())
    gx, gs = o.chscale_bwd(g(gy), g(x), sd, s_bs, relu_x=relu_x)
    rx, rs, A = R.chscale_grads(gy, x, s, relu_x)
    assert rel(gx, rx) < 1e-6 and rel(gs, rs) < 1e-5
    if relu_x:
        masked = ~(x > 0)
        assert int(masked.sum()) > 0 and bool((gx.cpu()[masked] == 0).all())
    elem("D", f"chscale_bwd gx {where}", gx, rx, U * rx.abs())
    elem("D", f"chscale_bwd gs {where}", gs, rs, (T / 64 + 8) * U * A)


# ------------------------------------------------------------------------------------------------ E. roi_align
def roi_window(T):
    """The window the engine chooses: W = 6 around the two middle rows."""
    return (T - 1) // 2 - 2, 6


def check_roi(o, name, z, rois, gy, windowed):
    B, C, T = z.shape
    out, (ref, mag) = o.roi_align_fwd(g(z), rois.to(DEV)), R.roi_align(z, rois)
    assert out.shape == ref.shape and rel(out, ref) < 1e-6
    elem("E", f"roi_align_fwd {name} C={C} T={T}", out, ref, 4 * U * mag)
    gz, (gref, A) = o.roi_align_bwd(g(gy), rois.to(DEV), T), R.roi_align_transpose(gy, rois, T)
    assert gz.shape == gref.shape and rel(gz, gref) < 1e-5
    r0, r1, _, _ = R.roi_rows(T)
    off = torch.ones(T, dtype=torch.bool)
    off[[r0, r1]] = False
    assert bool((gz.cpu()[:, :, off] == 0).all()), "roi_align_bwd: a row outside the two middle ones is not exactly 0"
    elem("E", f"roi_align_bwd {name} C={C} T={T}", gz, gref, (112 / 64 + 8) * U * A)
    if windowed:
        t0, W = roi_window(T)
        assert t0 >= 0 and t0 + W <= T and t0 <= r0 and r1 < t0 + W
        outw = o.roi_align_fwd(g(z[:, :, t0:t0 + W]), rois.to(DEV), T, t0)
        assert torch.equal(outw, out)
        gzw = o.roi_align_bwd(g(gy), rois.to(DEV), T, W, t0)
        assert gzw.shape == (B, C, W) and torch.equal(gzw, gz[:, :, t0:t0 + W])


@pytest.mark.parametrize("C", [5, 130])
def test_roi_align_golden(golden_dir, C):
    """roi_align_fwd_kernel and roi_align_bwd_kernel on every recorded table of tests/golden/roi_cases.npz."""
    o = ops()
    z = np.load(f"{golden_dir}/roi_cases.npz")
    for name in sorted({k.split(":")[0] for k in z.files}):
        rois = torch.from_numpy(z[f"{name}:rois"])
        B, T = rois.shape[0], int(z[f"{name}:L"]) // 4
        check_roi(o, name, rnd(B, C, T, seed=2500), rois, rnd(B, C, R.N_SEG, R.ROI_BINS, seed=2501), windowed=False)


@pytest.mark.parametrize("C", [5, 130])
@pytest.mark.parametrize("L", ROI_L)
def test_roi_align_synth(L, C):
    """synth.make_rois at T = 1, 2, 3 (one row; two half taps; one row with a weightless neighbour), 125 (odd) and 250
    (even); at the last two also the windowed forms (zT, t_off) with the engine's window."""
    o = ops()
    from electrocardio_panorama_amd import synth
    B, T = 3, L // 4
    rois = torch.from_numpy(synth.make_rois(np.random.default_rng(3), B, L))
    check_roi(o, f"synth L={L}", rnd(B, C, T, seed=2510), rois, rnd(B, C, R.N_SEG, R.ROI_BINS, seed=2511), windowed=T >= 125)


# ------------------------------------------------------------------------------------------------ F. window crop / scatter
def windows(T):
    mid = ((T - 1) // 2 - 2, 6) if T >= 12 else ((T - 1) // 2 - 1, 3)
    return [(0, 1), (0, 6), (T - 6, 6), (T - 1, 1), mid]


@pytest.mark.parametrize("B,G,Cg,T", [(3, 2, 6, 250), (2, 1, 5, 7)])
def test_window_crop_scatter(B, G, Cg, T):
    """window_crop_kernel and window_scatter_kernel, exact: W = 1, windows at t0 = 0 and ending at T, T < 64, on both halves
    of a two-halves-per-group view."""
    o = ops()
    from electrocardio_panorama_amd.ops import GV
    x = rnd(B, G * 2 * Cg, T, seed=2600)                     # [B, G, 2 halves, Cg, T]
    xd = g(x)
    halves = x.view(B, G, 2, Cg, T)
    for t0, W in windows(T):
        assert 0 <= t0 and t0 + W <= T
        for h in (0, 1):
            where = f"{(B, G, Cg, T)} window {(t0, W)} half {h}"
            crop = o.window_crop(GV(xd, B, G, Cg, T, 2 * G * Cg * T, 2 * Cg * T, h * Cg * T), t0, W)
            want = halves[:, :, h, :, t0:t0 + W].reshape(B, G * Cg, W)
            assert crop.shape == want.shape and torch.equal(crop.cpu(), want), where
            dst = torch.full((B, G * 2 * Cg, T), 7.0, device=DEV)
            o.window_scatter(crop, GV(dst, B, G, Cg, T, 2 * G * Cg * T, 2 * Cg * T, h * Cg * T), t0)
            got = dst.cpu().view(B, G, 2, Cg, T)
            assert bool((got[:, :, 1 - h] == 7.0).all()), where
            assert torch.equal(got[:, :, h, :, t0:t0 + W].reshape(B, G * Cg, W), want), where
            rest = got[:, :, h].clone()
            rest[..., t0:t0 + W] = 0
            assert float(rest.abs().max()) == 0.0, where
            elem("F", f"window_scatter {where}", got[:, :, h, :, t0:t0 + W].reshape(B, G * Cg, W), want, 0.0)


# ------------------------------------------------------------------------------------------------ seed search (CPU)
def _search(shape, start=2000, tries=200):
    for s in range(start, start + tries):
        c = R.oc_case(shape, s)
        R._OC.clear()
        if R.pro_margin(c["x"], c["pro"]) >= MARGIN:
            return s
    raise SystemExit(f"no seed for {shape}")


if __name__ == "__main__":      # CPU only: print a SEEDS table whose inputs clear the tie screen
    for k in SEEDS:
        print(f"    {k}: {_search(k)},")
