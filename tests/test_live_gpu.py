"""Live extents on the GPU: the convs behind the bias-free stem skip the column tiles that lie in a beat's all-zero
tail.  Every comparison is torch.equal between the promise handed over and not (ops.LIVE off, or live=None): same bits is the bar."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from electrocardio_panorama_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def split_fp16_forced():
    """Bare ops calls with the shape rules alone deciding (no batch hint left over from a model-level test) and the split-fp16
    kernels at these small batches: the forms the full-size step runs."""
    o = ops()
    saved = o.BATCH_HINT, o._H2_MIN_WGS, o.LIVE, o.LIVE_WGRAD
    o.BATCH_HINT, o._H2_MIN_WGS, o.LIVE, o.LIVE_WGRAD = None, 0, True, True
    yield
    o.BATCH_HINT, o._H2_MIN_WGS, o.LIVE, o.LIVE_WGRAD = saved


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


# ------------------------------------------------------------------------------------------------ the extent
def live_rule(e, L):
    cj = min(L // 2, (e + 6) // 2 + 1) if e else 0
    return min(L // 4, cj // 2 + 1) if cj else 0


@pytest.mark.parametrize("L", [8, 512, 5000])
@pytest.mark.parametrize("aligned", [True, False])
def test_live_extent_rows(L, aligned):
    """nef_live_extent against numpy on an all-zero row, a full row, a -0.0 tail, a NaN as the last live element and extents 1 .. 40;
    then the property it stands for: ops.stem_fwd's output is exactly zero at every t >= live."""
    o = ops()
    V = 3
    ext = [0, L, L // 2, L // 2] + [min(e, L) for e in range(1, 41)]
    while len(ext) % V:
        ext.append(L - 1)
    rows = len(ext)
    x = np.random.RandomState(7).randn(rows, L).astype(np.float32)
    x[x == 0] = 1.0
    for r, e in enumerate(ext):
        x[r, e:] = 0.0
    x[2, L // 2:] = -0.0                     # a negative-zero tail counts as zero
    x[3, L // 2 - 1] = np.nan                # ... and a NaN as non-zero
    want = np.array([live_rule(e, L) for e in ext], np.int32).reshape(rows // V, V)
    buf = torch.zeros(rows * L + 4, device=DEV)
    off = 0 if aligned else 1                # (a row start that is not 16-byte aligned: the scalar loads)
    xt = buf[off:off + rows * L].view(rows // V, V, L)
    xt.copy_(torch.from_numpy(x).view(rows // V, V, L))
    live = o.live_extent(xt)
    assert live.dtype == torch.int32 and tuple(live.shape) == (rows // V, V)
    assert np.array_equal(live.cpu().numpy(), want), (live.cpu().numpy(), want)
    w = rnd(128 * V, 1, 15, seed=11, scale=0.3)
    xs = xt.clone()
    xs[1, 0, L // 2 - 1] = 1.0               # (the NaN would spread over its row's outputs: the property is about finite rows)
    lv = o.live_extent(xs).cpu().numpy()
    y = o.stem_fwd(xs, w).view(rows // V, V, 128, L // 4)
    for b in range(rows // V):
        for v in range(V):
            assert not bool(y[b, v, :, int(lv[b, v]):].any()), (b, v, int(lv[b, v]))
    assert bool(y[0, 1].any())               # (the full row is not zero)


# ------------------------------------------------------------------------------------------------ forward / backward-data convs
B, G, T = 3, 3, 600                          # three 256-column tiles, the last ragged
EXT = [[0, 100, 300], [600, 100, 300], [600, 0, 300]]      # per (sample, group): tiles 0 / 1 / 2 / 3 live of 3


def zero_tail(x, ext):
    x = x.clone().view(B, G, -1, T)
    for b in range(B):
        for g_ in range(G):
            x[b, g_, :, ext[b][g_]:] = 0.0
    return x.view(B, -1, T)


def combos(o, Cin, Cout, wp):
    from electrocardio_panorama_amd.ops import GV
    res = GV.dense(rnd(B, G * Cout, T, seed=21), G)
    gate = GV.dense(rnd(B, G * Cout, T, seed=22), G)
    e_in = (rnd(B, G, Cin, seed=23) + 0.3, G * Cin, Cin)
    e_out = (rnd(B, G, Cout, seed=24) + 0.3, G * Cout, Cout)
    yield "res_relu_dropout", dict(res=res, relu=True, drop_p=0.2, drop_scale=1.25, seed=1234), None
    yield "gate_scale", dict(gate=gate, gate_scale=1.25), None
    yield "in_scale_res_scale", dict(in_scale=e_in, res=res, res_scale=e_out), None
    slots = o.conv_stats_buffer(wp, B, G, Cout, T, torch.device(DEV))
    assert slots is not None
    yield "gate_rowscale_stats1", dict(gate=gate, gate_rowscale=e_out, stats=slots, stats_mode=1), slots


@pytest.mark.parametrize("K,Cin,Cout,bias,add", [(7, 128, 128, False, 0), (7, 128, 128, False, 9), (3, 128, 128, False, 0),
                                                  (3, 64, 128, False, 0), (3, 128, 64, False, 2), (1, 64, 128, True, 0),
                                                  (7, 64, 64, False, 0)])
def test_conv_live_same_bits(K, Cin, Cout, bias, add):
    """The plain split-fp16 forms (128-row and 64-row tiles) with and without the promise: outputs, statistics slots and the
    x_amax_next word, for every epilogue option a launch of the step combines.  Everything but the operand (residual, gate, bias)
    is non-zero in the dead tiles, so their epilogue has real work to get right."""
    o = ops()
    from electrocardio_panorama_amd.ops import GV
    if not o.h2_ok(K, Cin, Cout, T):
        pytest.skip("split-fp16 convs switched off")
    x = zero_tail(rnd(B, G * Cin, T, seed=20), EXT)
    w = rnd(G * Cout, Cin, K, seed=25, scale=0.05)
    bv = rnd(G * Cout, seed=26, scale=0.2) if bias else None
    wp = o.pack_weight(w, G, T=T, plain=False)
    assert getattr(wp, "nef_wino", 0) == 3
    table = (torch.tensor(EXT, dtype=torch.int32) - add).to(DEV)
    st = o._amax_state(x.device)
    for name, kw, slots in combos(o, Cin, Cout, wp):
        got = []
        for live in ((table, add), None):
            if slots is not None:
                slots[0].fill_(float("nan"))
            y = o.conv(GV.dense(x, G), wp, Cout, K, bias=bv, live=live, **kw)
            word = st["nxt"][st["index"][(None, "conv")]].clone()
            got.append((y, word, slots[0].clone() if slots is not None else None))
        (y1, a1, s1), (y0, a0, s0) = got
        assert torch.equal(y1, y0), (name, float((y1 - y0).abs().max()))
        assert torch.equal(a1, a0) and float(a0) > 0, (name, float(a1), float(a0))
        if slots is not None:
            assert torch.equal(s1, s0) and not bool(torch.isnan(s0).any()), name
    # the module switch: with ops.LIVE off the promise is not handed on (the parent's entry point, unchanged)
    o.LIVE = False
    try:
        y2 = o.conv(GV.dense(x, G), wp, Cout, K, bias=bv, live=(table, add))
    finally:
        o.LIVE = True
    assert torch.equal(y2, o.conv(GV.dense(x, G), wp, Cout, K, bias=bv))


def test_conv_live_promise_is_what_skips():
    """The promise is USED: on an operand that breaks it, the dead tiles come out as if the operand were zero there.  Extent 0 leaves
    the first tile live (its window starts at t0 - PAD < 0): that one is computed from the real operand."""
    o = ops()
    from electrocardio_panorama_amd.ops import GV
    if not o.h2_ok(3, 128, 128, T):
        pytest.skip("split-fp16 convs switched off")
    x = rnd(B, G * 128, T, seed=30)
    w = rnd(G * 128, 128, 3, seed=31, scale=0.05)
    wp = o.pack_weight(w, G, T=T, plain=False)
    table = torch.zeros(B, G, dtype=torch.int32, device=DEV)
    y = o.conv(GV.dense(x, G), wp, 128, 3, live=(table, 0), x_scale=1.0)
    full = o.conv(GV.dense(x, G), wp, 128, 3, x_scale=1.0)
    assert torch.equal(y[:, :, :256], full[:, :, :256]) and bool(full[:, :, 256:].any())
    assert not bool(y[:, :, 256:].any())


# ------------------------------------------------------------------------------------------------ weight gradients
B5 = 5
EXT5 = EXT + [[100, 600, 0], [300, 300, 600]]


@pytest.mark.parametrize("K,Cin,Cout", [(7, 128, 128), (3, 128, 128), (3, 64, 128)])
@pytest.mark.parametrize("side", ["gradient", "input", "both"])
def test_conv_bwd_weight_live_same_bits(K, Cin, Cout, side):
    """Form 3 (the producer / consumer kernel) with and without the promise.  T = 600 is ten 64-column items per sample, the last
    ragged; 42 shares of two items each, so share boundaries fall everywhere in the live / dead pattern.  Plain random data.
    `both`: input and gradient share the tail, as in every launch the train step wires -- gw AND both magnitude words are equal.
    `gradient`: only gy is zero from the extent on (addend 0);  `input`: only x is (addend PAD: an item's window starts at t0 - PAD).
    There the OTHER operand is non-zero in the dead items: gw must still be the same, and so must the promised operand's word.  The
    other operand's word is the exception the header states: it is taken over the live items, so it is at most the full launch's
    and equals that operand's largest element outside the dead items -- checked against exactly that."""
    o = ops()
    from electrocardio_panorama_amd.ops import GV
    if not o.h2w_ok(K, Cin, Cout, T):
        pytest.skip("split-fp16 weight gradient switched off")
    PAD = (K - 1) // 2

    def tail(t, add):
        t = t.clone().view(B5, G, -1, T)
        for b in range(B5):
            for g_ in range(G):
                t[b, g_, :, max(EXT5[b][g_] + add, 0):] = 0.0
        return t.view(B5, -1, T)

    x, gy = rnd(B5, G * Cin, T, seed=40), rnd(B5, G * Cout, T, seed=41, scale=1e-2)
    if side == "gradient":
        gy, add = tail(gy, 0), 0
    elif side == "input":
        x, add = tail(x, 0), PAD
    else:
        x, gy, add = tail(x, 0), tail(gy, PAD), PAD
    table = torch.tensor(EXT5, dtype=torch.int32).to(DEV)
    st = o._amax_state(x.device)
    got = []
    for live in ((table, add), None):
        gw = o.conv_bwd_weight(GV.dense(x, G), GV.dense(gy, G), K, live=live, h2=True)
        i = st["index"][(None, "bww")]
        got.append((gw, st["nxt"][i:i + 2].clone()))
    (g1, a1), (g0, a0) = got
    assert torch.equal(g1, g0), float((g1 - g0).abs().max())
    assert bool(g0.any()) and bool((a0 > 0).all())
    if side == "both":
        assert torch.equal(a1, a0), (a1, a0)
    else:
        # the staged part of the other operand: live items are the 64-column tiles t0 < extent + addend; x is staged with its window
        def live_max(t, halo):
            t = t.view(B5, G, -1, T)
            m = torch.zeros((), device=DEV)
            for b in range(B5):
                for g_ in range(G):
                    n = max(EXT5[b][g_] + add, 0)
                    end = min(T, (n + 63) // 64 * 64 + halo) if n else 0
                    if end:
                        m = torch.maximum(m, t[b, g_, :, :end].abs().max())
            return m
        if side == "gradient":      # words: [x, gy]
            assert torch.equal(a1[1], a0[1]) and float(a1[0]) <= float(a0[0])
            lo, hi = live_max(x, 0), live_max(x, 4)      # (the staged window reaches up to 4 columns past the item)
            assert float(lo) <= float(a1[0]) <= float(hi), (float(lo), float(a1[0]), float(hi))
        else:
            assert torch.equal(a1[0], a0[0]) and float(a1[1]) <= float(a0[1])
            assert float(a1[1]) == float(live_max(gy, 0)), (float(a1[1]), float(live_max(gy, 0)))


def test_conv_bwd_weight_live_promise_is_what_skips():
    """The promise is USED: extent 0 with addend 0 declares every item dead (an item's test is t0 >= bound, and 0 >= 0), so on
    operands that break the promise the gradient comes out exactly zero, where the full launch's is not."""
    o = ops()
    from electrocardio_panorama_amd.ops import GV
    if not o.h2w_ok(3, 128, 128, T):
        pytest.skip("split-fp16 weight gradient switched off")
    x, gy = rnd(B, G * 128, T, seed=50), rnd(B, G * 128, T, seed=51, scale=1e-2)
    table = torch.zeros(B, G, dtype=torch.int32, device=DEV)
    gw = o.conv_bwd_weight(GV.dense(x, G), GV.dense(gy, G), 3, live=(table, 0), h2=True, x_scale=1.0, gy_scale=64.0)
    full = o.conv_bwd_weight(GV.dense(x, G), GV.dense(gy, G), 3, h2=True, x_scale=1.0, gy_scale=64.0)
    assert bool(full.any()) and not bool(gw.any())
    # ... and one live item per row (extent 1): only the first 64 columns contribute
    gy1 = gy.clone()
    gy1[:, :, 64:] = 0.0
    one = o.conv_bwd_weight(GV.dense(x, G), GV.dense(gy, G), 3, live=(table + 1, 0), h2=True, x_scale=1.0, gy_scale=64.0)
    want = o.conv_bwd_weight(GV.dense(x, G), GV.dense(gy1, G), 3, h2=True, x_scale=1.0, gy_scale=64.0)
    assert torch.equal(one, want)


# ------------------------------------------------------------------------------------------------ the whole step
class Cfg(dict):
    __getattr__ = dict.__getitem__


def make_cfg(V, lr=0.1):
    return Cfg(MODEL=Cfg(model="model_nefnet", theta_L=1, loss="v1", resume=""), DATA=Cfg(lead_num=V, noise=False),
               SOLVER=Cfg(optim="sgd", lr=lr, scheduler="MultiStep", lr_step=[50, 100], reg_loss="l1_loss", loss_using=[1, 2, 3],
                          loss_factor=[0.5, 0.5, 1], epochs=1),
               output_dir="/tmp/nef_test", desc="debug")


def hashed_model(V):
    from electrocardio_panorama_amd.network import build_model
    from oracle import hashweights as hw
    m = build_model(make_cfg(V)).float()
    m.load_state_dict({**hw.hashed_params(V), **hw.hashed_buffers()})
    return m.to(DEV)


def batch(L, kind):
    from electrocardio_panorama_amd import synth
    b = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in synth.make_batch(4, 3, L, seed=123).items()}
    if kind == "no_tail":
        b["data"] = torch.where(b["data"] == 0, torch.full_like(b["data"], 0.01), b["data"])
    elif kind == "zero_sample":
        b["data"][1] = 0.0
    return b


def run_steps(b, graphed, live_on):
    """Two train steps (dropout on) from the hashed weights: losses, every gradient, the BatchNorm buffers, the updated parameters."""
    o = ops()
    from electrocardio_panorama_amd.graph import GraphedTrainStep
    from electrocardio_panorama_amd.network import build_loss
    from electrocardio_panorama_amd.solver.optim_scheduler import get_optimizer
    cfg = make_cfg(3)
    saved = o._H2_MIN_WGS, o.LIVE
    o._H2_MIN_WGS, o.LIVE = 0, live_on      # the split-fp16 convs of the full-size step, at this small batch
    try:
        m = hashed_model(3).train()
        m.dropout_p = 0.2
        random.seed(5)
        out = []
        if graphed:
            step = GraphedTrainStep(m, cfg)
            for _ in range(2):
                out.append(step(b["data"], b["input_theta"], b["target_theta"], b["rois"], b["target_view"]).clone())
                out.append(step.flat_g.clone())
        else:
            lossf, optim = build_loss(cfg), get_optimizer(cfg, m.parameters())
            for _ in range(2):
                ov = m(b["data"], b["input_theta"], b["target_theta"], b["rois"], phase="train")
                ls = lossf(ov[0], ov[1], ov[2], b["target_view"].unsqueeze(1), cfg)
                ls[0].backward()
                out += [x.detach().clone() for x in ls]
                out += [p.grad.detach().clone() for _, p in sorted(m.named_parameters()) if p.grad is not None]
                optim.step()
                optim.zero_grad()
        torch.cuda.synchronize()
        out += [v.detach().clone() for _, v in sorted(m.state_dict().items())]
        return out
    finally:
        o._H2_MIN_WGS, o.LIVE = saved


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
@pytest.mark.parametrize("L,kind", [(3000, "tail"), (2048, "tail"), (3000, "no_tail"), (3000, "zero_sample")])
def test_train_step_live_same_bits(L, kind, graphed):
    o = ops()
    b = batch(L, kind)
    lv = o.live_extent(b["data"])
    if kind == "tail" and L == 3000:      # the case is what it says: the third 256-column tile of every row is dead, the chain's
        assert int(lv.max()) + 24 <= 512, int(lv.max())      # + 12 + 2 + 1 and a conv's own PAD included
    elif kind == "tail":                  # T = 512: the extents (260 .. 291) end just inside the second of two tiles -- all live
        assert 256 < int(lv.min()) and int(lv.max()) < 512
    elif kind == "no_tail":
        assert int(lv.min()) == L // 4
    else:
        assert int(lv[1].max()) == 0
    on, off = run_steps(b, graphed, True), run_steps(b, graphed, False)
    assert len(on) == len(off) and len(on) > 40
    for i, (x, y) in enumerate(zip(on, off)):
        assert x.shape == y.shape and torch.equal(x, y), (i, tuple(x.shape))
    assert all(bool(torch.isfinite(x).all()) for x in on[:2])
