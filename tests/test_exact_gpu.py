"""Every conv form bit for bit on lattice data (tests/lattice_ref.py).

tests/test_ops_gpu.py compares through a rel-L2 over the whole tensor (1e-5 forward, 1e-4 gradients): that catches a wrong kernel, not
a wrong ELEMENT -- one tap column missing at one tile seam of the (3, 1, 64, 128, 5000, 2) backward-data case moves it by 9e-5.  Here
the operands sit on a small dyadic lattice (x, gy in {+-1, +-2}, w in {+-0.5, +-1}, scales 0.5 / 1 / 2 / 1.25), so every product is
exact in fp32 and in fp16 x fp16 -> fp32, every partial sum is an integer number of grid steps far below 2^24 (asserted from the
reference alone, lattice_ref.precheck), and a kernel that multiplies the right pairs must reproduce the fp64 convolution BIT FOR
BIT in any summation order: `torch.equal` is the assertion, the first differing index the diagnosis.  A ReLU, gate or dropout
decision on an exact value is the same decision on both sides, so there is no tie screen.

Dyadic forms (exact): the direct fp32 kernel; Winograd F(2,3) for K = 3 (transforms of +-1 and 0.5); the split-fp16 direct kernel
with its power-of-two row, launch and rescue scales, long rows and packed short rows; the polyphase form (0.25 / 0.75 phase weights)
and its edge kernels; the direct, split-fp16 and polyphase weight gradients; stem, convt2, upsample2, lead_mean, mix_fwd.
Forms whose transforms are NOT dyadic run the same cases under `max |y - ref| < step / 4` and `round(y / grid) == ref / grid`
(a structural error is >= step; the project's recorded error of these forms, 4..10e-7 rel-L2, is ~1e-4 absolute here): F(4,3)
(1/4, 1/6, 1/24 ...), the K = 7 member of the F(2,.) family (conv_mfma.hip's header: F(2,4) on taps 0..3, "entries up to 3 and
4/3", u2 = (..) / 6), and the transposed F(3,4) / F(4,4)+F(3,4) weight gradients with their LDS-DMA form (1/6, 1/12, 1/24, 1/45).
Their measured worst |y - ref| / step is reported per form through conftest.report, never used as a bar.

Every case names the form it expects and asserts that the dispatcher picked it (the packed operand's nef_wino, the shape rules
h2_ok / wino_ok / h2w_ok / poly_*_ok, the wino= / h2= arguments of conv_bwd_weight, the restated host rules lattice_ref.direct_wide /
wgrad_dma / test_lengths_gpu.stem_bwd_kernel); a case whose form is unavailable fails.  The polyphase forms take T / 2 even only:
T = 258 and 514 assert that refusal and hold the split-fp16 upsampling-prologue form, which those rows run on, to the same reference.

BatchNorm-backward slot sums: with dyadic statistics (mean in {-1, 0, 1}, invstd in {0.5, 1, 2}) xhat is on the lattice as well, so
sum g m AND sum g m xhat are in the exact set.

Wrong-on-purpose edits tried against this file on the MI355X (none is committed; each drops or doubles a read, none moves a store;
all five in one library, 94 of the 276 tests failed, the other 182 passed), and what caught them:

1. conv_h2_kernel, long rows: staged position r = 0 of every tile (the left halo column) forced to zero.
   test_split_fp16 K = 3 and K = 7 at T = 258 and 514 -- "first at (b, channel, t) = (0, 0, 256), t % 256 = 0: expected 37, got 11 grid
   units" -- and not at T <= 256, where the tile's left halo is the conv's own zero padding; K = 1 (r = 0 is column 0 itself) at every
   T.  Also test_prologues[split-fp16, mode 1, T = 258] (modes 2 / 3 stage intervals through other code and pass),
   test_epilogues_and_views[split-fp16, T = 258], test_split_fp16_row_scaled_epilogues[T = 258], test_slot_sums[split-fp16].
2. conv_h2_kernel, packed short rows: the first of the four gap positions behind a sample staged with the sample's last column
   instead of zero (a gap one position short).  test_split_fp16_packed_short_rows, K = 3 at every T, already at B = 1 -- "first at
   (0, 0, 7), t % 12 = 7: expected 24, got 42 grid units"; K = 1 has no neighbour taps and passes.
3. conv_fwd_kernel: the staging guard `t < T` written `t < T - 1` (the last input column is never read).  All 34 test_direct_fp32
   cases -- "first at (0, 0, 125), t % 128 = 125: expected -59, got 0" --, test_prologues[direct], test_epilogues_and_views[direct]
   (and [F(2,3), T = 130], whose backward-data launch falls to the direct kernel), test_convt2[matrix cores].
4. poly_fwd_edge_kernel: the store of the last column's correction removed.  test_polyphase, all six cases that take the form:
   "polyphase forward, last column ... 377 of 384 elements wrong".
5. convt2_bwd_weight_kernel: `b += 2 * CT_SPLIT`.  test_convt2[B = 33, fma] alone -- "convt2_bwd_weight (33, 2, 16, 'fma'): 31498
   of 32768 elements wrong" --; B = 1 and 5 never take the loop's second trip and pass.
"""
import contextlib

import pytest
import torch

import lattice_ref as R
from lattice_ref import DIRECT, F23, F43, H2

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORM_NAME = {DIRECT: "direct fp32", F23: "Winograd F(2,3)", F43: "Winograd F(4,3)", H2: "split-fp16"}
WORST = {}      # non-dyadic forms: worst |y - ref| / step seen, per form


def ops():
    from electrocardio_panorama_amd import ops as o
    return o


def GV():
    from electrocardio_panorama_amd.ops import GV as gv
    return gv


def d(t):
    """An fp64 lattice tensor on the device in fp32 (exact: the lattice has a handful of bits)."""
    if t is None:
        return None
    if t.dtype == torch.uint8:
        return t.to(DEV).contiguous()
    f = t.float()
    assert torch.equal(f.double(), t)
    return f.to(DEV).contiguous()


@contextlib.contextmanager
def algo(h2, wino):
    """The dispatch switches of one case: set, then restored (not test_ops_gpu's autouse fixture)."""
    o = ops()
    saved = (o.H2, o.WINOGRAD, o.BATCH_HINT)
    o.H2, o.WINOGRAD, o.BATCH_HINT = bool(h2), bool(wino), None
    try:
        yield o
    finally:
        o.H2, o.WINOGRAD, o.BATCH_HINT = saved


ALGO = {DIRECT: (False, False), F23: (False, True), F43: (False, True), H2: (True, True)}


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    import conftest
    for form in sorted(WORST):
        conftest.report(f"lattice cases, {form}: worst |y - ref| / step = {WORST[form]:.2e} (bar 0.25, a structural error is >= 1)")


def _where(idx, axes, tile, t_off=0):
    idx = [int(i) for i in idx]
    if axes[-1] == "t":
        idx[-1] += t_off                      # (a slice of columns compared on its own)
    s = "(" + ", ".join(axes) + ") = " + str(tuple(idx))
    if tile and axes[-1] == "t":
        s += f", t % {tile} = {idx[-1] % tile}"
    return s


def _fail(form, case, bad, got, want, grid, axes, tile, extra="", t_off=0):
    idx = bad.nonzero()[0]
    e, g = float(want[tuple(idx)]) / grid, float(got[tuple(idx)]) / grid
    pytest.fail(f"{form} {case}: {int(bad.sum())} of {bad.numel()} elements wrong{extra}; first at {_where(idx, axes, tile, t_off)}: "
                f"expected {e:g}, got {g:g} grid units (grid {grid:g})")


def exact(form, case, got, ref, grid, tile=None, axes=("b", "channel", "t"), t_off=0):
    """torch.equal against the fp64 reference cast to fp32."""
    want = ref.float()
    assert torch.equal(want.double(), ref), "the reference itself is not an fp32 number"
    got = got.detach().float().cpu()
    assert got.shape == want.shape, (form, case, got.shape, want.shape)
    if not torch.equal(got, want):
        _fail(form, case, ~(got == want), got.double(), ref, grid, axes, tile, t_off=t_off)


def near(form, case, got, ref, grid, step, tile=None, axes=("b", "channel", "t")):
    """The bar of the non-dyadic forms: every element within step / 4 and on the reference's grid point."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (form, case, got.shape, ref.shape)
    err = (got - ref).abs()
    finite = bool(torch.isfinite(got).all())
    worst = float(err.max()) / step if finite else float("inf")
    WORST[form] = max(WORST.get(form, 0.0), worst)
    bad = ~(err < step / 4) | (torch.round(got / grid) != ref / grid)
    if bool(bad.any()):
        _fail(form, case, bad, got, ref, grid, axes, tile, f" (worst |y - ref| = {worst:.3g} step, bar 0.25)")


def check(form_id, K, case, got, ref, grid, step, tile=None):
    """Exact for the dyadic forms, step / 4 for F(4,3) and for K = 7 through the F(2,.) family."""
    if form_id == F43:
        near(f"Winograd F(4,3), K = {K}", case, got, ref, grid, step, tile)
    elif form_id == F23 and K == 7:
        near("Winograd F(2,4)+F(2,3), K = 7", case, got, ref, grid, step, tile)
    else:
        exact(FORM_NAME[form_id], case, got, ref, grid, tile)


def packed(o, w, G, flip, T, form, f4=False, plain=True):
    """pack_weight + the assertion that the dispatcher picked `form` for this launch."""
    wp = o.pack_weight(w, G, flip=flip, T=T, f4=f4, plain=plain)
    got = int(getattr(wp, "nef_wino", 0))
    assert got == form, f"expected {FORM_NAME[form]}, the dispatcher picked {FORM_NAME.get(got, got)}"
    return wp


def launch(o, L, wp, G, Cout, K, flip, **kw):
    return o.conv(GV().dense(d(L["x"]), G), wp, Cout, K, role="conv_bwd_data" if flip else "conv_fwd", **kw)


# ------------------------------------------------------------------------------------------------ direct fp32
@pytest.mark.parametrize("K,G,Cin,Cout,T,B,how", R.DIRECT_CASES)
def test_direct_fp32(K, G, Cin, Cout, T, B, how):
    """conv_fwd_kernel, forward and backward-data: one sample per 128-column tile from T = 128, several per tile below; with
    split-fp16 and Winograd switched off, and at the T that fall to it by the shape rules with both on."""
    with algo(how == "on", how == "on") as o:
        for flip in (False, True):
            ci, co = (Cout, Cin) if flip else (Cin, Cout)
            if how == "on":
                assert not o.h2_ok(K, ci, co, T) and not o.wino_ok(K, ci, co, T)
            L = R.conv_launch(K, G, ci, co, T, B, flip=flip, seed=K * 1000 + T)
            wp = packed(o, d(L["w"]), G, flip, T, DIRECT)
            if G == 28 and not flip:
                assert R.direct_wide(G, co, T, B)               # the 128-row tile
            else:
                assert not R.direct_wide(G, co, T, B)
            y = launch(o, L, wp, G, co, K, flip)
            exact(FORM_NAME[DIRECT], ("bwd-data" if flip else "fwd", K, G, ci, co, T, B, how), y, L["ref"], L["grid"], R.NT)


# ------------------------------------------------------------------------------------------------ Winograd
@pytest.mark.parametrize("form", [F23, F43])
@pytest.mark.parametrize("K,G,Cin,Cout,T,B,flip", R.WINO_CASES)
def test_winograd(K, G, Cin, Cout, T, B, flip, form):
    """conv_wino_kernel (F(2,3): K = 3 exact, K = 7 through F(2,4)+F(2,3) at step / 4) and conv_wino4_kernel (F(4,3), step / 4)."""
    with algo(*ALGO[form]) as o:
        assert o.wino_ok(K, Cin, Cout, T)
        L = R.conv_launch(K, G, Cin, Cout, T, B, flip=flip, seed=K * 1000 + T, wino23=(K == 3))
        wp = packed(o, d(L["w"]), G, flip, T, form, f4=(form == F43))
        y = launch(o, L, wp, G, Cout, K, flip)
        check(form, K, ("bwd-data" if flip else "fwd", K, G, Cin, Cout, T, B), y, L["ref"], L["grid"], L["step"], tile=R.NT)


@pytest.mark.parametrize("K,G,Cin,Cout,T,B", R.ZERO_TAIL_CASES)
def test_winograd_f2_keeps_exact_zeros_over_a_zero_tail(K, G, Cin, Cout, T, B):
    """ops.py's reason for keeping the encoder on the F(2,.) forms: input rows that end in exact zeros (a beat's tail) give exactly
    0.0 there, because every product only sees the receptive field of the outputs it feeds -- K = 3 and K = 7 (F(2,4)+F(2,3))."""
    with algo(*ALGO[F23]) as o:
        L = R.conv_launch(K, G, Cin, Cout, T, B, seed=77, tail_zeros=R.ZERO_TAIL, wino23=(K == 3))
        wp = packed(o, d(L["w"]), G, False, T, F23)
        y = launch(o, L, wp, G, Cout, K, False)
        t0 = T - R.ZERO_TAIL + K // 2
        tail = y[:, :, t0:].cpu()
        if not bool((tail == 0).all()):
            bad = tail != 0
            idx = bad.nonzero()[0]
            pytest.fail(f"Winograd F(2,.) K={K}: {int(bad.sum())} of {bad.numel()} outputs over the zero tail are not 0.0; first at "
                        f"(b, channel, t) = ({int(idx[0])}, {int(idx[1])}, {t0 + int(idx[2])}): {float(tail[tuple(idx)])!r}")
        check(F23, K, ("zero tail", K, G, Cin, Cout, T, B), y, L["ref"], L["grid"], L["step"], tile=R.NT)


# ------------------------------------------------------------------------------------------------ split-fp16 direct
@pytest.mark.parametrize("K,G,Cin,Cout,T,B", R.H2_CASES)
def test_split_fp16(K, G, Cin, Cout, T, B):
    """conv_h2_kernel, 256-output tiles, 64- and 128-channel tiles: explicit scale, measured scale, a launch forced into the range
    rescue (one element x 2^12 after its site measured), and a backward-data launch on a gradient x 2^-20."""
    seed = K * 1000 + T + Cout
    case = (K, G, Cin, Cout, T, B)
    with algo(*ALGO[H2]) as o:
        assert o.h2_ok(K, Cin, Cout, T)
        o.h2_clamped()
        L = R.conv_launch(K, G, Cin, Cout, T, B, seed=seed)
        wd = d(L["w"])
        wp = packed(o, wd, G, False, T, H2)
        exact("split-fp16, explicit scale", case, launch(o, L, wp, G, Cout, K, False, x_scale=2.0 ** 7), L["ref"], L["grid"], R.NTO)
        exact("split-fp16, measured scale", case, launch(o, L, wp, G, Cout, K, False), L["ref"], L["grid"], R.NTO)
        # range rescue: the site measured amax = 2 (scale 2^7: 2 -> 2^8); an element of 1 or 2 times 2^12 lands at 2^19 or 2^20, past
        # fp16's 65504, and the tile that holds it redoes itself with its own scale
        S = R.conv_launch(K, G, Cin, Cout, T, B, seed=seed, spike=(12345, 2.0 ** 12))
        assert float(S["x"].abs().max()) in (2.0 ** 12, 2.0 ** 13) and torch.equal(S["w"], L["w"])
        with o.amax_scope(o.new_amax_scope()):
            wps = packed(o, wd, G, False, T, H2)
            exact("split-fp16, site's first launch", case, launch(o, L, wps, G, Cout, K, False), L["ref"], L["grid"], R.NTO)
            o.amax_roll()
            exact("split-fp16, range rescue", case, launch(o, S, wps, G, Cout, K, False), S["ref"], S["grid"], R.NTO)
            o.amax_roll()
        Gd = R.conv_launch(K, G, Cin, Cout, T, B, flip=True, seed=seed, x_mul=2.0 ** -20)
        wf = packed(o, d(Gd["w"]), G, True, T, H2)
        exact("split-fp16 bwd-data, gradient x 2^-20, measured", case, launch(o, Gd, wf, G, Cout, K, True), Gd["ref"], Gd["grid"], R.NTO)
        exact("split-fp16 bwd-data, gradient x 2^-20, explicit", case, launch(o, Gd, wf, G, Cout, K, True, x_scale=2.0 ** 27),
              Gd["ref"], Gd["grid"], R.NTO)
        assert o.h2_clamped() == 0


@pytest.mark.parametrize("K,G,Cin,Cout,T", R.PACKED_CASES)
def test_split_fp16_packed_short_rows(K, G, Cin, Cout, T):
    """conv_h2_kernel PACK: spt = 260 // (T + 4) samples per tile at a pitch of T + 4; B = 1, spt, spt + 1, 2 spt + 1 (one sample, a
    full tile, a tile + 1, two tiles + 1).  A tap that leaks across the zero gap between two samples changes an integer."""
    spt, batches = R.packed_batches(T)
    with algo(*ALGO[H2]) as o:
        assert o._h2_packed(K, T)
        for B in batches:
            for flip in (False, True):
                ci, co = (Cout, Cin) if flip else (Cin, Cout)
                assert o.h2_ok(K, ci, co, T)
                L = R.conv_launch(K, G, ci, co, T, B, flip=flip, seed=K * 100 + T + B)
                wp = packed(o, d(L["w"]), G, flip, T, H2)
                y = launch(o, L, wp, G, co, K, flip)
                exact("split-fp16 packed short rows", ("bwd-data" if flip else "fwd", K, G, ci, co, T, f"B={B}", f"spt={spt}"), y,
                      L["ref"], L["grid"], T + 4)


# ------------------------------------------------------------------------------------------------ prologues
@pytest.mark.parametrize("form", [DIRECT, F23, F43, H2])
@pytest.mark.parametrize("mode,G,Cig,Cog,T", R.PROLOGUE_CASES)
def test_prologues(mode, G, Cig, Cog, T, form):
    """BatchNorm affine + ReLU (bit 0) and x2 upsampling (bit 1) while the conv stages its input: three passes of Bp = 2 with their
    own affine, forward on every form that takes a prologue and the weight gradient with the same modes (direct, split-fp16, and --
    under the F(4,3) parameter -- the transposed F(3,4) form, which runs on the LDS-DMA kernel wherever nef_bww_glds_ok says so)."""
    P, Bp = 3, 2
    c = R.prologue_case(mode, G, Cig, Cog, T, P, Bp, seed=mode * 1000 + T, wino23=(form == F23))
    case = ("mode", mode, G, Cig, Cog, T)
    with algo(*ALGO[form]) as o:
        pro = (mode, d(c["a"]) if mode & 1 else None, d(c["b"]) if mode & 1 else None, Bp)
        if form == H2:
            assert o.h2_ok(3, Cig, Cog, T, mode) and o.h2w_ok(3, Cig, Cog, T, mode, False)
        elif form != DIRECT:
            assert o.wino_ok(3, Cig, Cog, T, mode)
        wp = packed(o, d(c["w"]), G, False, T, form, f4=(form == F43), plain=False)
        xv = GV().dense(d(c["x"]), G)
        y = o.conv(xv, wp, Cog, 3, bias=d(c["bias"]), pro=pro)
        check(form, 3, ("fwd",) + case, y, c["ref"], c["grid"], c["step"], tile=R.TILE[form])
        gv = GV().dense(d(c["gy"]), G)
        axes = ("co", "ci", "k")
        if form == DIRECT:
            gw = o.conv_bwd_weight(xv, gv, 3, pro=pro, wino=False, h2=False)
            exact("direct fp32 weight gradient", case, gw, c["gw"], c["gw_grid"], axes=axes)
        elif form == H2:
            gw = o.conv_bwd_weight(xv, gv, 3, pro=pro, h2=True)
            exact("split-fp16 weight gradient", case, gw, c["gw"], c["gw_grid"], axes=axes)
        elif form == F43:
            dma = R.wgrad_dma(3, Cig, Cog, T, mode, False, P)
            assert dma == (not (mode & 2 and T % 4))
            gw = o.conv_bwd_weight(xv, gv, 3, pro=pro, wino=4)
            near("transposed F(3,4) weight gradient" + (", LDS-DMA" if dma else ""), case, gw, c["gw"], c["gw_grid"], c["gw_step"], axes=axes)


# ------------------------------------------------------------------------------------------------ epilogues and views
@pytest.mark.parametrize("form", [DIRECT, F23, H2])
@pytest.mark.parametrize("T,which", R.EPILOGUE_CASES)
def test_epilogues_and_views(T, which, form):
    """test_conv_epilogue_and_views' chain: bias, in_scale through a strided half view, residual, ReLU, a replayed mask with scale
    1.25, a gate with scale 1.25; the weight gradient through the same view + in_scale; backward-data written into one half of a full
    tensor whose other half keeps its fill value."""
    B, V, K = 2, 3, 3
    c = R.epilogue_case(T, which, B, V, K, seed=T + which, wino23=(form == F23))
    case = ("T", T, "half", which)
    with algo(*ALGO[form]) as o:
        encd, scd, wd, gyd = d(c["enc"]), d(c["scale"]), d(c["w"]), d(c["gy"])
        insc = (scd.view(-1)[which * 64:], 128 * V, 128)
        wp = packed(o, wd, V, False, T, form, plain=False)
        y = o.conv(GV().half(encd, V, which), wp, 128, K, bias=d(c["bias"]), in_scale=insc, res=GV().dense(d(c["res"]), V),
                   gate=GV().dense(d(c["gate"]), V), gate_scale=R.GATE_SCALE, relu=True, mask=d(c["mask"]), drop_scale=R.DROP_SCALE)
        exact(FORM_NAME[form] + " epilogue chain", case, y, c["ref"], c["grid"], R.TILE[form])
        axes = ("co", "ci", "k")
        if form == F23:       # (in_scale keeps the transposed F(3,4) form off the LDS-DMA kernel)
            assert not R.wgrad_dma(K, 64, 128, T, 0, True)
            gw = o.conv_bwd_weight(GV().half(encd, V, which), GV().dense(gyd, V), K, in_scale=insc, wino=4)
            near("transposed F(3,4) weight gradient", case, gw, c["gw"], c["gw_grid"], c["gw_step"], axes=axes)
        else:
            if form == H2:
                assert o.h2w_ok(K, 64, 128, T, 0, True)
            gw = o.conv_bwd_weight(GV().half(encd, V, which), GV().dense(gyd, V), K, in_scale=insc, wino=None if form == H2 else False,
                                   h2=(form == H2))
            exact(("split-fp16" if form == H2 else "direct fp32") + " weight gradient, half view + in_scale", case, gw, c["gw"],
                  c["gw_grid"], axes=axes)
        # backward-data (128 -> 64 channels per group: F(2,3) takes it from T = 256, shorter rows stay on the direct kernel)
        bform = form if (form != F23 or T >= 256) else DIRECT
        wf = packed(o, wd, V, True, T, bform)
        full = torch.full((B, 128 * V, T), 7.0, device=DEV)
        o.conv(GV().dense(gyd, V), wf, 64, K, out=GV().half(full, V, which), role="conv_bwd_data")
        got = full.cpu().view(B, V, 2, 64, T)
        exact(FORM_NAME[bform] + " bwd-data into a half view", case, got[:, :, which].reshape(B, 64 * V, T), c["gx"], c["gx_grid"],
              R.TILE[bform])
        assert bool((got[:, :, 1 - which] == 7.0).all()), "the other half lost its fill value"


@pytest.mark.parametrize("B,G,C,T", R.SCALED_BLOCK_CASES)
def test_split_fp16_row_scaled_epilogues(B, G, C, T):
    """The split-fp16 kernel's own epilogue options, in test_conv_h2_channel_scaled_block_input's setup: res_scale on the residual, and
    the gated backward-data launch with gate_rowscale whose slots carry sum_t (ungated gradient) x gate (stats_mode 1, read back
    through slots_to_rows)."""
    c = R.scaled_block_case(B, G, C, T, seed=T)
    case = (B, G, C, T)
    with algo(*ALGO[H2]) as o:
        wd, ed = d(c["w"]), d(c["e"])
        sc = (ed, G * C, C)
        wp = packed(o, wd, G, False, T, H2, plain=False)
        y = o.conv(GV().dense(d(c["h"]), G), wp, C, 3, res=GV().dense(d(c["x"]), G), relu=True, res_scale=sc)
        exact("split-fp16 res_scale", case, y, c["y"], c["grid"], R.NTO)
        wf = packed(o, wd, G, True, T, H2, plain=False)
        slots = o.conv_stats_buffer(wf, B, G, C, T, torch.device(DEV))
        assert slots is not None
        slots[0].fill_(float("nan"))
        g = o.conv(GV().dense(d(c["gc"]), G), wf, C, 3, res=GV().dense(d(c["g2"]), G), role="conv_bwd_data", gate=GV().dense(d(c["xr"]), G),
                   gate_rowscale=sc, stats=slots, stats_mode=1)
        exact("split-fp16 gate_rowscale", case, g, c["gated"], c["g_grid"], R.NTO)
        exact("split-fp16 stats_mode 1 rows", case, o.slots_to_rows(slots, B), c["rows"], c["r_grid"], axes=("b", "channel"))


# ------------------------------------------------------------------------------------------------ slot sums
def _slots(sl, nslot, B):
    """The slot tensor [C, B * nslot, 2] as [B, C, nslot, 2] on the CPU."""
    C = sl.shape[0]
    return sl.detach().cpu().view(C, B, nslot, 2).permute(1, 0, 2, 3).contiguous()


def _pad_slots(ref, nslot):
    B, C, n, _ = ref.shape
    assert nslot >= n
    out = torch.zeros(B, C, nslot, 2, dtype=ref.dtype)
    out[:, :, :n] = ref
    return out


@pytest.mark.parametrize("form", [H2, F43])
@pytest.mark.parametrize("G,Cin,Cout,T,B", R.SLOT_CASES)
def test_slot_sums(G, Cin, Cout, T, B, form):
    """nef_conv_args.stats (sum y, sum y^2 per 128-column slot) and bnb (sum g m, sum g m xhat of the layer below a backward-data
    launch), slot by slot.  Split-fp16: exact, both words.  F(4,3): its outputs carry the transforms' rounding, so sum y and both bnb
    words sit under step / 4 per slot, and sum y^2 is held to the kernel's OWN outputs: |slot - sum y_gpu^2| <= 127 * 2^-24 * sum
    y_gpu^2, the worst case of adding 128 non-negative fp32 numbers in any order (a dropped column is caught by sum y beside it)."""
    case = (G, Cin, Cout, T, B)
    with algo(*ALGO[form]) as o:
        takes = form == H2 or o.wino_ok(3, Cin, Cout, T)
        assert takes == (form == H2 or Cout % 128 == 0 or T >= 256), case
        if not takes:       # 64 output channels under T = 256: no F(4,3) tile, and the boundary says so instead of leaving no sums
            L = R.slot_case(G, Cin, Cout, T, B, seed=T)
            wp = packed(o, d(L["w"]), G, False, T, DIRECT, f4=True, plain=False)
            assert o.conv_stats_buffer(wp, B, G, Cout, T, torch.device(DEV)) is None
            return
        name = FORM_NAME[form]
        L = R.slot_case(G, Cin, Cout, T, B, seed=T)
        wp = packed(o, d(L["w"]), G, False, T, form, f4=True, plain=False)
        slots = o.conv_stats_buffer(wp, B, G, Cout, T, torch.device(DEV))
        assert slots is not None
        slots[0].fill_(float("nan"))
        y = launch(o, L, wp, G, Cout, 3, False, stats=slots)
        check(form, 3, ("fwd + stats",) + case, y, L["ref"], L["grid"], L["step"], tile=R.TILE[form])
        got, want = _slots(slots[0], slots[1], B), _pad_slots(L["slots"], slots[1])
        axes = ("b", "channel", "slot")
        if form == H2:
            exact(name + " slot sum y", case, got[..., 0], want[..., 0], L["grid"], axes=axes)
            exact(name + " slot sum y^2", case, got[..., 1], want[..., 1], L["grid"] ** 2, axes=axes)
        else:
            near(name + " slot sum y", case, got[..., 0], want[..., 0], L["grid"], L["step"], axes=axes)
            own = _pad_slots(R.slot_sums(y.double().cpu()), slots[1])[..., 1]
            err = (got[..., 1].double() - own).abs()
            assert bool((err <= 127 * 2.0 ** -24 * own).all()), (name, case, float((err / own.clamp_min(1e-30)).max()))
        # backward-data launch + the BatchNorm-backward sums of the layer below, three passes
        Lb = R.slot_case(G, Cin, Cout, T, B, flip=True, seed=T, P=3)
        wf = packed(o, d(Lb["w"]), G, True, T, form, f4=True, plain=False)
        slots = o.conv_stats_buffer(wf, B, G, Cout, T, torch.device(DEV))
        assert slots is not None
        slots[0].fill_(float("nan"))
        bnb = tuple(d(Lb[k]) for k in ("xb", "mean", "invstd", "a", "b")) + (Lb["Bp"], slots)
        gx = launch(o, Lb, wf, G, Cout, 3, True, bnb=bnb)
        check(form, 3, ("bwd-data + bnb",) + case, gx, Lb["ref"], Lb["grid"], Lb["step"], tile=R.TILE[form])
        got, want = _slots(slots[0], slots[1], B), _pad_slots(Lb["bnb"], slots[1])
        g1 = R.grid_of(want[..., 1])
        if form == H2:
            exact(name + " bnb sum g m", case, got[..., 0], want[..., 0], Lb["grid"], axes=axes)
            exact(name + " bnb sum g m xhat", case, got[..., 1], want[..., 1], g1, axes=axes)
        else:
            near(name + " bnb sum g m", case, got[..., 0], want[..., 0], Lb["grid"], Lb["step"], axes=axes)
            near(name + " bnb sum g m xhat", case, got[..., 1], want[..., 1], g1, Lb["step"] * 0.5, axes=axes)      # |xhat| >= 0.5


# ------------------------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize("K,G,Cig,Cog,T", R.WGRAD_CASES)
def test_weight_gradients(K, G, Cig, Cog, T):
    """conv_bwd_weight_kernel (direct fp32), conv_h2w (split-fp16, with and without in_scale), and at step / 4 the transposed
    F(3,4) / F(4,4)+F(3,4) forms: on the LDS-DMA kernel without in_scale, on conv_bwd_weight_kernel with it.  B = 1, 2, 5 split
    unevenly over the sample shares."""
    axes = ("co", "ci", "k")
    with algo(*ALGO[H2]) as o:
        for B in R.WGRAD_BATCHES:
            for insc in (False, True):
                c = R.wgrad_case(K, G, Cig, Cog, T, B, seed=K * 1000 + T + B, insc=insc)
                case = (K, G, Cig, Cog, T, f"B={B}", "in_scale" if insc else "plain")
                xv, gv = GV().dense(d(c["x"]), G), GV().dense(d(c["gy"]), G)
                sc = (d(c["sc"]), G * Cig, Cig) if insc else None
                if not insc:
                    gw = o.conv_bwd_weight(xv, gv, K, wino=False, h2=False)
                    exact("direct fp32 weight gradient", case, gw, c["ref"], c["grid"], axes=axes)
                assert o.h2w_ok(K, Cig, Cog, T, 0, insc)
                gw = o.conv_bwd_weight(xv, gv, K, in_scale=sc, h2=True)
                exact("split-fp16 weight gradient", case, gw, c["ref"], c["grid"], axes=axes)
                dma = R.wgrad_dma(K, Cig, Cog, T, 0, insc)
                assert dma == (not insc)
                gw = o.conv_bwd_weight(xv, gv, K, in_scale=sc, wino=4)
                near(f"transposed {'F(3,4)' if K == 3 else 'F(4,4)+F(3,4)'} weight gradient" + (", LDS-DMA" if dma else ""), case, gw,
                     c["ref"], c["grid"], c["step"], axes=axes)


@pytest.mark.parametrize("K,T,B,G,C", R.WGRAD_DMA_CASES)
def test_weight_gradient_dma_edges(K, T, B, G, C):
    """The LDS-DMA kernel at test_conv_bwd_weight_dma_edges' shapes (tiles that reach outside [0, T), chunks that reach outside the
    operand), on the lattice."""
    with algo(*ALGO[F43]) as o:
        assert R.wgrad_dma(K, C, C, T)
        c = R.wgrad_case(K, G, C, C, T, B, seed=K * 1000 + T)
        gw = o.conv_bwd_weight(GV().dense(d(c["x"]), G), GV().dense(d(c["gy"]), G), K, wino=4)
        near(f"transposed {'F(3,4)' if K == 3 else 'F(4,4)+F(3,4)'} weight gradient, LDS-DMA", (K, T, B, G, C), gw, c["ref"], c["grid"],
             c["step"], axes=("co", "ci", "k"))


# ------------------------------------------------------------------------------------------------ polyphase
@pytest.mark.parametrize("G,Cig,Cog,T,B,aff", R.POLY_CASES)
def test_polyphase(G, Cig, Cog, T, B, aff):
    """conv1d(upsample2(prologue(x)), w) in polyphase form: conv_poly_fwd (+ nef_poly_fwd_edge), conv_bwd_data_poly on the interleaved
    and on the phase-major gradient (+ nef_poly_bwd_edge), conv_bwd_weight_poly (+ nef_poly_wgrad_fold).  The first and the last
    column -- the edge kernels' -- are compared on their own first.  The phase split needs T / 2 even: T = 258 and 514 assert the
    refusal and run the form those rows take instead (the split-fp16 kernel's upsampling prologue)."""
    P = 3
    c = R.poly_case(G, Cig, Cog, T, B, aff, seed=T + aff, P=P)
    case = (G, Cig, Cog, T, B, "affine" if aff else "plain")
    takes = (T // 2) % 2 == 0
    with algo(*ALGO[H2]) as o:
        assert o.poly_fwd_ok(G, Cog, Cig, T) == takes and o.poly_bwd_ok(G, Cog, Cig, T) == takes
        pro = (3, d(c["a"]), d(c["b"]), c["Bp"]) if aff else (2, None, None, 1)
        xv, wd = GV().dense(d(c["x"]), G), d(c["w"])
        axes = ("co", "ci", "k")
        if not takes:
            assert not o.poly_w_ok(B, G, Cog, Cig, T)
            wp = packed(o, wd, G, False, T, H2, plain=False)
            y = o.conv(xv, wp, Cog, 3, bias=d(c["bias"]), pro=pro)
            exact("split-fp16 upsampling prologue", case, y, c["ref"], c["grid"], R.NTO)
            gw = o.conv_bwd_weight(xv, GV().dense(d(c["gy"]), G), 3, pro=pro, h2=True)
            exact("split-fp16 weight gradient, upsampling prologue", case, gw, c["gw"], c["gw_grid"], axes=axes)
            return
        y = o.conv_poly_fwd(xv, wd, Cog, bias=d(c["bias"]), pro=pro, save_edge=True)
        exact("polyphase forward, first column", case, y[:, :, :1], c["ref"][:, :, :1], c["grid"])
        exact("polyphase forward, last column", case, y[:, :, T - 1:], c["ref"][:, :, T - 1:], c["grid"], t_off=T - 1)
        exact("polyphase forward", case, y, c["ref"], c["grid"], 2 * R.NTO)
        gyd = d(c["gy"])
        gpm = d(R.phase_major(c["gy"]))
        for name, gx in (("interleaved", o.conv_bwd_data_poly(GV().dense(gyd, G), wd, Cig)),
                         ("phase-major", o.conv_bwd_data_poly(GV().dense(gpm, G), wd, Cig, phase_major=True))):
            exact(f"polyphase backward-data ({name}), first column", case, gx[:, :, :1], c["gx"][:, :, :1], c["gx_grid"])
            exact(f"polyphase backward-data ({name}), last column", case, gx[:, :, T // 2 - 1:], c["gx"][:, :, T // 2 - 1:], c["gx_grid"],
                  t_off=T // 2 - 1)
            exact(f"polyphase backward-data ({name})", case, gx, c["gx"], c["gx_grid"], R.NTO)
        assert o.poly_w_ok(B, G, Cog, Cig, T) == (T % 4 == 0)
        gw = o.conv_bwd_weight_poly(xv, gpm, Cog, pro, y.nef_xedge)
        exact("polyphase weight gradient", case, gw, c["gw"], c["gw_grid"], axes=axes)


# ------------------------------------------------------------------------------------------------ related kernels
@pytest.mark.parametrize("B,V,L", R.STEM_SHAPES)
def test_stem(B, V, L):
    """stem_fwd and both stem weight-gradient kernels at test_lengths_gpu's small shapes (first maximum wins in the pool, on both
    sides: lattice data is full of ties and needs no screen)."""
    from test_lengths_gpu import STEM_MFMA, STEM_VALU, stem_bwd_kernel
    o = ops()
    kernel = stem_bwd_kernel(L)
    assert kernel == (STEM_MFMA if (B, V, L) in ((2, 1, 8), (258, 1, 8)) else STEM_VALU)
    c = R.stem_case(B, V, L, seed=L)
    exact("stem_fwd", (B, V, L), o.stem_fwd(d(c["x"]), d(c["w"])), c["ref"], c["grid"], 63)
    exact(kernel, (B, V, L), o.stem_bwd_weight(d(c["x"]), d(c["w"]), d(c["gy"])), c["gw"], c["gw_grid"], axes=("channel", "1", "k"))


@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("B,G,T", R.CONVT2_CASES)
def test_convt2(B, G, T, fma):
    """ConvTranspose1d(k = 2, s = 2) on both routes (1x1 conv on the matrix cores + interleave; the plain-FMA kernels).  B = 33: the
    CT_SPLIT = 32 sample loop of convt2_bwd_weight_kernel takes a second trip."""
    c = R.convt2_case(B, G, T, seed=B)
    case = (B, G, T, "fma" if fma else "matrix cores")
    with algo(*ALGO[H2]) as o:
        exact("convt2_fwd", case, o.convt2_fwd(d(c["x"]), d(c["w"]), d(c["bias"]), G, fma=fma), c["ref"], 0.5)
        exact("convt2_bwd_data", case, o.convt2_bwd_data(d(c["gy"]), d(c["w"]), G, fma=fma), c["gx"], 0.5)
        gw, gb = o.convt2_bwd_weight(d(c["x"]), d(c["gy"]), G, fma=fma)
        exact("convt2_bwd_weight", case, gw, c["gw"], 1.0, axes=("ci", "co", "j"))
        exact("convt2_bwd_weight bias", case, gb, c["gb"], 1.0, axes=("channel",))


@pytest.mark.parametrize("Tin", R.UPSAMPLE_TIN)
def test_upsample2(Tin):
    """upsample2_fwd, and upsample2_bwd on both kernels (row form for even Tin >= 4, the generic one otherwise)."""
    o = ops()
    x, gy = R.lat((2, 5, Tin), R.X_VALS, Tin), R.lat((2, 5, 2 * Tin), R.X_VALS, Tin + 1)
    rows = Tin % 2 == 0 and Tin >= 4
    assert rows == (Tin in (4, 516))
    exact("upsample2_fwd", Tin, o.upsample2_fwd(d(x)), R.upsample2(x), 0.25)
    exact("upsample2_bwd_rows" if rows else "upsample2_bwd_kernel", Tin, o.upsample2_bwd(d(gy)), R.upsample2_bwd(gy), 0.25)


@pytest.mark.parametrize("V", R.MIX_V)
def test_lead_mean_and_mix(V):
    """lead_mean (a division by V = 1, 2, 4, 8: exact) and mix_fwd."""
    o = ops()
    B, T, c1, c2 = 3, 7, V - 1, 0
    z1, z2r, q = R.lat((B, 128 * V, T), R.X_VALS, V), R.lat((B, 128 * V, T), R.X_VALS, V + 1), R.lat((B, 256), R.R_VALS, V + 2)
    lm = R.lead_mean(z1, z2r, V)
    lat_d = o.lead_mean(d(z1), d(z2r), V)
    exact("lead_mean", V, lat_d, lm, 1.0 / V)
    exact("mix_fwd", V, o.mix_fwd(lat_d, d(z1), d(z2r), d(q), V, c1, c2), R.mix(lm, z1, z2r, q, V, c1, c2), 0.5 / V)
