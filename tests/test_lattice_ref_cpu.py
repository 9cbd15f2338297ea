"""The exact-arithmetic reference of tests/test_exact_gpu.py, checked without a GPU:

1. on every case of the GPU file the fp64 reference equals torch's own fp32 CPU op bit for bit (so "bit for bit against fp64" asks
   of a HIP kernel nothing that a plain fp32 implementation in another summation order does not deliver), and the preconditions --
   grid, units < 2^24, fp16-exact operands, step -- hold (lattice_ref asserts them wherever a case is built);
2. one product dropped at a seam moves exactly the expected element, by at least `step`: the seam element is recomputed here as an
   explicit sum over (channel, tap), which also anchors the reference's own indexing at the tile seams.
"""
import pytest
import torch

import lattice_ref as R


def f32(*ts):
    return [None if t is None else t.float() for t in ts]


def same(a32, ref64):
    assert a32.dtype == torch.float32 and ref64.dtype == torch.float64
    return torch.equal(a32.double(), ref64)


# ------------------------------------------------------------------------------------------------ 1. fp32 torch == fp64, every case
@pytest.mark.parametrize("K,G,Cin,Cout,T,B,algo", R.DIRECT_CASES)
def test_direct_cases(K, G, Cin, Cout, T, B, algo):
    for flip in (False, True):
        ci, co = (Cout, Cin) if flip else (Cin, Cout)
        L = R.conv_launch(K, G, ci, co, T, B, flip=flip, seed=K * 1000 + T)
        x, w = f32(L["x"], L["w"])
        assert same(R.conv_bwd_data(x, w, G) if flip else R.conv(x, w, G), L["ref"])
        assert L["units"] < 2 ** 16 and L["step"] == 0.5


@pytest.mark.parametrize("K,G,Cin,Cout,T,B,flip", R.WINO_CASES)
def test_winograd_cases(K, G, Cin, Cout, T, B, flip):
    L = R.conv_launch(K, G, Cin, Cout, T, B, flip=flip, seed=K * 1000 + T, wino23=(K == 3))
    x, w = f32(L["x"], L["w"])
    assert same(R.conv_bwd_data(x, w, G) if flip else R.conv(x, w, G), L["ref"])


@pytest.mark.parametrize("K,G,Cin,Cout,T,B", R.ZERO_TAIL_CASES)
def test_zero_tail_cases(K, G, Cin, Cout, T, B):
    L = R.conv_launch(K, G, Cin, Cout, T, B, seed=77, tail_zeros=R.ZERO_TAIL, wino23=(K == 3))
    assert same(R.conv(*f32(L["x"], L["w"]), G), L["ref"])
    tail = L["ref"][:, :, T - R.ZERO_TAIL + K // 2:]
    assert tail.numel() and bool((tail == 0).all())
    assert bool((L["ref"][:, :, T - R.ZERO_TAIL + K // 2 - 1] != 0).any())       # the column before it still sees data


@pytest.mark.parametrize("K,G,Cin,Cout,T,B", R.H2_CASES)
def test_split_fp16_cases(K, G, Cin, Cout, T, B):
    seed = K * 1000 + T + Cout
    for kw in (dict(), dict(spike=(12345, 2.0 ** 12)), dict(flip=True, x_mul=2.0 ** -20)):
        L = R.conv_launch(K, G, Cin, Cout, T, B, seed=seed, **kw)
        x, w = f32(L["x"], L["w"])
        assert same(R.conv_bwd_data(x, w, G) if kw.get("flip") else R.conv(x, w, G), L["ref"])


@pytest.mark.parametrize("K,G,Cin,Cout,T", R.PACKED_CASES)
def test_packed_cases(K, G, Cin, Cout, T):
    spt, batches = R.packed_batches(T)
    assert spt == 260 // (T + 4)
    for B in batches:
        for flip in (False, True):
            L = R.conv_launch(K, G, Cin, Cout, T, B, flip=flip, seed=K * 100 + T + B)
            x, w = f32(L["x"], L["w"])
            assert same(R.conv_bwd_data(x, w, G) if flip else R.conv(x, w, G), L["ref"])


@pytest.mark.parametrize("mode,G,Cig,Cog,T", R.PROLOGUE_CASES)
def test_prologue_cases(mode, G, Cig, Cog, T):
    c = R.prologue_case(mode, G, Cig, Cog, T, seed=mode * 1000 + T, wino23=True)
    x, a, b, w, bias, gy = f32(c["x"], c["a"], c["b"], c["w"], c["bias"], c["gy"])
    xin = R.prologue(x, mode, a, b, 2)
    assert same(xin, c["xin"])
    assert same(R.conv(xin, w, G, bias), c["ref"]) and same(R.conv_bwd_weight(xin, gy, G, 3), c["gw"])


@pytest.mark.parametrize("T,which", R.EPILOGUE_CASES)
def test_epilogue_cases(T, which):
    c = R.epilogue_case(T, which, seed=T + which, wino23=True)
    xs, w, bias, res, gate, gy = f32(c["xs"], c["w"], c["bias"], c["res"], c["gate"], c["gy"])
    y, _ = R.epilogue(R.conv(xs, w, 3, bias), res=res, relu=True, mask=c["mask"], drop_scale=R.DROP_SCALE, gate=gate,
                      gate_scale=R.GATE_SCALE)
    assert same(y, c["ref"])
    assert same(R.conv_bwd_weight(xs, gy, 3, 3), c["gw"]) and same(R.conv_bwd_data(gy, w, 3), c["gx"])


@pytest.mark.parametrize("B,G,C,T", R.SCALED_BLOCK_CASES)
def test_scaled_block_cases(B, G, C, T):
    c = R.scaled_block_case(B, G, C, T, seed=T)
    x, h, e, w, gc, g2, xr = f32(c["x"], c["h"], c["e"], c["w"], c["gc"], c["g2"], c["xr"])
    assert same(R.epilogue(R.conv(h, w, G), res=x, res_scale=e, relu=True)[0], c["y"])
    gated, pre = R.epilogue(R.conv_bwd_data(gc, w, G), res=g2, gate=xr, gate_scale=1.0, gate_rowscale=e)
    assert same(gated, c["gated"]) and same((pre * xr).sum(2), c["rows"])


@pytest.mark.parametrize("G,Cin,Cout,T,B", R.SLOT_CASES)
def test_slot_cases(G, Cin, Cout, T, B):
    L = R.slot_case(G, Cin, Cout, T, B, seed=T)
    y = R.conv(*f32(L["x"], L["w"]), G)
    assert same(R.slot_sums(y), L["slots"])
    assert torch.equal(L["slots"].sum(2)[..., 0], L["ref"].sum(2))
    L = R.slot_case(G, Cin, Cout, T, B, flip=True, seed=T, P=3)
    g, xb, mean, invstd, a, b = f32(L["ref"], L["xb"], L["mean"], L["invstd"], L["a"], L["b"])
    assert same(R.bn_backward_sums(g, xb, mean, invstd, a, b, L["Bp"]), L["bnb"])


@pytest.mark.parametrize("K,G,Cig,Cog,T", R.WGRAD_CASES)
def test_wgrad_cases(K, G, Cig, Cog, T):
    for B in R.WGRAD_BATCHES:
        for insc in (False, True):
            c = R.wgrad_case(K, G, Cig, Cog, T, B, seed=K * 1000 + T + B, insc=insc)
            xin, gy = f32(c["xin"], c["gy"])
            assert same(R.conv_bwd_weight(xin, gy, G, K), c["ref"])
            assert c["units"] < 2 ** 16 and c["step"] >= 0.5


@pytest.mark.parametrize("K,T,B,G,C", R.WGRAD_DMA_CASES)
def test_wgrad_dma_cases(K, T, B, G, C):
    assert R.wgrad_dma(K, C, C, T)
    c = R.wgrad_case(K, G, C, C, T, B, seed=K * 1000 + T)
    assert same(R.conv_bwd_weight(*f32(c["xin"], c["gy"]), G, K), c["ref"])


@pytest.mark.parametrize("G,Cig,Cog,T,B,aff", R.POLY_CASES)
def test_poly_cases(G, Cig, Cog, T, B, aff):
    c = R.poly_case(G, Cig, Cog, T, B, aff, seed=T + aff, P=3)
    x, w, bias, a, b, gy = f32(c["x"], c["w"], c["bias"], c["a"], c["b"], c["gy"])
    xp = R.prologue(x, 1, a, b, c["Bp"]) if aff else x
    u = R.upsample2(xp)
    assert same(R.conv(u, w, G, bias), c["ref"]) and same(R.conv_bwd_weight(u, gy, G, 3), c["gw"])
    assert same(R.upsample2_bwd(R.conv_bwd_data(gy, w, G)), c["gx"])
    # the written-out adjoint is autograd's
    xr = c["xp"].clone().requires_grad_(True)
    R.conv(R.upsample2(xr), c["w"], G).backward(c["gy"])
    assert torch.equal(xr.grad, c["gx"])
    gpm = R.phase_major(c["gy"])
    assert torch.equal(gpm.view(B, G * Cog, 2, T // 2).permute(0, 1, 3, 2).reshape(B, G * Cog, T), c["gy"])


@pytest.mark.parametrize("B,V,L", R.STEM_SHAPES)
def test_stem_cases(B, V, L):
    c = R.stem_case(B, V, L, seed=L)
    x, w, gy = f32(c["x"], c["w"], c["gy"])
    assert same(R.stem(x, w), c["ref"]) and same(R.stem_bwd_weight(x, w, gy), c["gw"])


@pytest.mark.parametrize("B,G,T", R.CONVT2_CASES)
def test_convt2_cases(B, G, T):
    c = R.convt2_case(B, G, T, seed=B)
    x, w, bias, gy = f32(c["x"], c["w"], c["bias"], c["gy"])
    assert same(R.convt2(x, w, bias, G), c["ref"])
    for got, want in zip(R.convt2_grads(x, w, bias, gy, G), (c["gx"], c["gw"], c["gb"])):
        assert same(got, want)


def test_elementwise_cases():
    for Tin in R.UPSAMPLE_TIN:
        x = R.lat((2, 5, Tin), R.X_VALS, Tin)
        gy = R.lat((2, 5, 2 * Tin), R.X_VALS, Tin + 1)
        assert same(R.upsample2(x.float()), R.upsample2(x))
        xr = x.clone().requires_grad_(True)
        R.upsample2(xr).backward(gy)
        assert torch.equal(R.upsample2_bwd(gy), xr.grad) and same(R.upsample2_bwd(gy.float()), xr.grad)
    for V in R.MIX_V:
        z1, z2r, q = R.lat((3, 128 * V, 7), R.X_VALS, V), R.lat((3, 128 * V, 7), R.X_VALS, V + 1), R.lat((3, 256), R.R_VALS, V + 2)
        lm = R.lead_mean(z1, z2r, V)
        assert same(R.lead_mean(z1.float(), z2r.float(), V), lm)
        assert same(R.mix(lm.float(), z1.float(), z2r.float(), q.float(), V, V - 1, 0), R.mix(lm, z1, z2r, q, V, V - 1, 0))
        assert R.grid_of(lm) >= 1.0 / V


# ------------------------------------------------------------------------------------------------ 2. one product dropped at a seam
def explicit_conv_element(x, w, G, b, co, t, drop=None):
    """sum over (ci, k) of w[co, ci, k] x[b, g Cin + ci, t + k - K // 2], written out; `drop` = (ci, k) leaves one product out."""
    Cout, Cin, K = w.shape[0] // G, w.shape[1], w.shape[2]
    g = co // Cout
    s, T = 0.0, x.shape[2]
    for k in range(K):
        tt = t + k - K // 2
        if 0 <= tt < T:
            for ci in range(Cin):
                if drop != (ci, k):
                    s += float(w[co, ci, k]) * float(x[b, g * Cin + ci, tt])
    return s


def seam_columns(T, tile):
    return sorted({t for t in (0, tile - 1, tile, 2 * tile - 1, 2 * tile, T - 1) if 0 <= t < T})


@pytest.mark.parametrize("K,T,tile,flip", [(3, 130, R.NT, False), (7, 258, R.NT, False), (3, 258, R.NTO, True), (7, 514, R.NTO, False),
                                            (1, 129, R.NT, True)])
def test_dropped_product_conv(K, T, tile, flip):
    G, Cin, Cout, B = 2, 64, 128, 2
    L = R.conv_launch(K, G, Cin, Cout, T, B, flip=flip, seed=5)
    w = L["weff"]
    for t in seam_columns(T, tile):
        b, co = B - 1, Cout + 3                                     # second group: a read across the group boundary would show
        assert explicit_conv_element(L["x"], w, G, b, co, t) == float(L["ref"][b, co, t])
        k = min(K - 1, T - 1 - t + K // 2)                          # a tap that is inside the row at this column
        wrong = L["ref"].clone()
        wrong[b, co, t] = explicit_conv_element(L["x"], w, G, b, co, t, drop=(Cin - 1, k))
        diff = (wrong - L["ref"]).abs()
        assert int((diff != 0).sum()) == 1 and float(diff[b, co, t]) >= L["step"]
        assert float(diff[b, co, t]) / L["grid"] >= 1.0             # at least one grid unit: torch.equal cannot miss it


def test_dropped_product_packed_gap():
    """Two samples of a packed short-row tile: a tap that leaks across the gap adds a foreign product to the first column."""
    K, G, Cin, Cout, T, B = 3, 2, 64, 128, 16, 3
    L = R.conv_launch(K, G, Cin, Cout, T, B, seed=6)
    leak = float(L["w"][0, 0, 0]) * float(L["x"][0, 0, T - 1])     # sample 0's last column under sample 1's first output
    assert abs(leak) >= L["step"] and abs(leak) / L["grid"] >= 1.0
    assert explicit_conv_element(L["x"], L["w"], G, 1, 0, 0) == float(L["ref"][1, 0, 0])


@pytest.mark.parametrize("K,T,B", [(3, 66, 2), (7, 130, 5), (3, 194, 1)])
def test_dropped_product_wgrad(K, T, B):
    G, Cig, Cog = 2, 64, 64
    c = R.wgrad_case(K, G, Cig, Cog, T, B, seed=7)
    co, ci = Cog + 1, Cig - 1
    for k in (0, K - 1):
        for t in seam_columns(T, R.WT):
            terms = [(bb, tt) for bb in range(B) for tt in range(T) if 0 <= tt + k - K // 2 < T]
            full = sum(float(c["gy"][bb, co, tt]) * float(c["xin"][bb, Cig + ci, tt + k - K // 2]) for bb, tt in terms)
            assert full == float(c["ref"][co, ci, k])
            if (B - 1, t) in terms:
                one = float(c["gy"][B - 1, co, t]) * float(c["xin"][B - 1, Cig + ci, t + k - K // 2])
                assert abs(one) >= c["step"] and abs(one) / c["grid"] >= 1.0


@pytest.mark.parametrize("T,aff", [(256, False), (260, True)])
def test_dropped_product_polyphase_edges(T, aff):
    G, Cig, Cog, B = 2, 64, 64, 3
    c = R.poly_case(G, Cig, Cog, T, B, aff, seed=8, P=3)
    u = R.upsample2(c["xp"])
    for t in (0, 1, T - 2, T - 1):                                  # the first and the last column are the edge kernels'
        b, co = B - 1, Cog + 2
        full = explicit_conv_element(u, c["w"], G, b, co, t) + float(c["bias"][co])
        assert full == float(c["ref"][b, co, t])
        nz = [ci for ci in range(Cig) if float(u[b, Cig + ci, t]) != 0.0]
        part = explicit_conv_element(u, c["w"], G, b, co, t, drop=(nz[-1], 1)) + float(c["bias"][co])
        assert abs(full - part) >= c["step"] and abs(full - part) / c["grid"] >= 1.0


def test_dropped_sample_convt2():
    """b += 2 * CT_SPLIT in the sample loop: sample 32 of 33 never enters the weight gradient."""
    c = R.convt2_case(33, 2, 16, seed=33)
    _, gw32, _ = R.convt2_grads(c["x"][:32], c["w"], c["bias"], c["gy"][:32], 2)
    diff = (gw32 - c["gw"]).abs()
    assert float((diff >= 1.0).double().mean()) > 0.5                # a whole sample's products: most elements move by >= one unit


def test_dropped_product_stem():
    c = R.stem_case(2, 1, 252, seed=9)
    x, w = c["x"], c["w"]
    conv = torch.nn.functional.conv1d(x, w, None, 2, 7, 1, 1)
    s = sum(float(w[5, 0, k]) * float(x[1, 0, 2 * 40 + k - 7]) for k in range(15))
    assert s == float(conv[1, 5, 40]) and abs(float(w[5, 0, 3]) * float(x[1, 0, 2 * 40 + 3 - 7])) >= c["step"]


def test_tables_cover_the_tiles():
    assert {T for *_, T, _, a in R.DIRECT_CASES if a == "off"} >= {1, 2, 7, R.NT - 2, R.NT - 1, R.NT, R.NT + 1, R.NT + 2, 2 * R.NT + 2}
    assert {c[4] for c in R.H2_CASES} >= {R.NTO - 2, R.NTO, R.NTO + 2, 2 * R.NTO + 2} and {c[3] for c in R.H2_CASES} == {64, 128}
    assert {c[4] for c in R.WGRAD_CASES} >= {R.WT, R.WT + 2, 2 * R.WT - 2, 2 * R.WT, 2 * R.WT + 2, 3 * R.WT + 2}
    assert any(R.direct_wide(G, Cout, T, B) for K, G, Cin, Cout, T, B, a in R.DIRECT_CASES)
    assert not R.direct_wide(2, 128, 258, 3) and R.direct_wide(28, 128, 258, 5)
    assert max(c[0] for c in R.CONVT2_CASES) > 32                   # CT_SPLIT: the sample loop's second trip
    for c in R.DIRECT_CASES + R.WINO_CASES + R.H2_CASES:
        assert c[4] <= 516 and 64 <= c[2] <= 256 and 64 <= c[3] <= 256
