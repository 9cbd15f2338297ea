"""Dead conv tiles ("Zero-fill exit"): a tile of a plain split-fp16 launch that lies in the operand's all-zero tail stores
its zeros and leaves where the launch's epilogue is known to keep them, and runs the full epilogue on zero accumulators where it is
not; the stem's matrix-core weight gradient stops every row at its extent.  Every comparison is torch.equal between ops.LIVE off
(the promise is dropped: the plain entry points) and the default; output buffers are filled with NaN before every launch, so the
comparison also proves that every output is written."""
import pytest
import torch
import torch.nn.functional as F

from util import GRAD_TOL, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, G, CIN = 8, 3, 64
NAN = float("nan")


def ops():
    from electrocardio_panorama_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def split_fp16_forced():
    """As tests/test_live_gpu.py: the shape rules alone decide, and the split-fp16 kernels run at these small batches."""
    o = ops()
    saved = o.BATCH_HINT, o._H2_MIN_WGS, o.LIVE, o.LIVE_WGRAD
    o.BATCH_HINT, o._H2_MIN_WGS, o.LIVE, o.LIVE_WGRAD = None, 0, True, True
    yield
    o.BATCH_HINT, o._H2_MIN_WGS, o.LIVE, o.LIVE_WGRAD = saved


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def extents(T):
    """Per (sample, group), mixed from {0, 100, 300, T}: with 256-column tiles and T = 600 / 602 that is 2 / 2 / 1 / 0 dead tiles of 3
    (the first tile of an extent-0 row stays live: its window starts at t0 - PAD < 0, tests/test_live_gpu.py pins that)."""
    v = [0, 100, 300, T]
    return [[v[(b + 2 * g_ + (b >> 2)) % 4] for g_ in range(G)] for b in range(B)]


def zero_tail(x, ext, add, T):
    x = x.clone().view(B, G, -1, T)
    for b in range(B):
        for g_ in range(G):
            x[b, g_, :, max(ext[b][g_] + add, 0):] = 0.0
    return x.view(B, -1, T)


def dead_mask(ext, add, pad, T):
    """[B, G, 1, T] bool: the columns of the tiles t0 with t0 - pad >= extent + add."""
    m = torch.zeros(B, G, 1, T, dtype=torch.bool)
    for b in range(B):
        for g_ in range(G):
            for t0 in range(0, T, 256):
                if t0 - pad >= ext[b][g_] + add:
                    m[b, g_, 0, t0:t0 + 256] = True
    return m.to(DEV)


def launch_pair(o, xv, wp, Cout, K, T, table, add, slots=None, **kw):
    """The same launch with ops.LIVE off and on, each into a NaN-filled output (and NaN-filled slots): (y, x_amax_next word, the
    x_clamped counter, slots) per setting."""
    from electrocardio_panorama_amd.ops import GV
    st = o._amax_state(xv.t.device)
    got = []
    for on in (False, True):
        o.LIVE = on
        try:
            y = torch.full((B, G * Cout, T), NAN, device=DEV)
            if slots is not None:
                slots[0].fill_(NAN)
            before = st["clamped"].clone()
            o.conv(xv, wp, Cout, K, out=GV.dense(y, G), live=(table, add), **kw)
            word = st["nxt"][st["index"][(None, "conv")]].clone()
            got.append((y, word, st["clamped"] - before, slots[0].clone() if slots is not None else None))
        finally:
            o.LIVE = True
    return got


def same(name, off, on):
    (y0, a0, c0, s0), (y1, a1, c1, s1) = off, on
    assert not bool(torch.isnan(y1).any()), name      # every output is written
    assert torch.equal(y1, y0), (name, float((y1 - y0).abs().max()))
    assert torch.equal(a1, a0) and float(a0) > 0, (name, float(a1), float(a0))
    assert torch.equal(c1, c0), name
    if s0 is not None:
        assert torch.equal(s1, s0) and not bool(torch.isnan(s0).any()), name


@pytest.mark.parametrize("T", [600, 602])      # 602: T % 4 == 2 -- a half-live quad ends every row, every other row is 8-byte aligned
@pytest.mark.parametrize("Cout", [128, 64])    # the 128-row tile (TM = 2) and the 64-row tile (TM = 1)
@pytest.mark.parametrize("K", [7, 3, 1])
def test_dead_tile_same_bits(K, Cout, T):
    """Every epilogue a launch of the step combines, on operands with mixed extents.  Which path a dead tile takes is told by the sign
    of its zeros under a negative gate scale (the full epilogue writes gate > 0 ? +0 * -s = -0.0, the exit writes +0.0): the exit is
    taken where it may be and nowhere else."""
    o = ops()
    from electrocardio_panorama_amd.ops import GV
    if not o.h2_ok(K, CIN, Cout, T):
        pytest.skip("split-fp16 convs switched off")
    PAD = (K - 1) // 2
    ext = extents(T)
    assert {e for row in ext for e in row} == {0, 100, 300, T}
    add = PAD                                            # the operand is a conv's output: its bound is the table + PAD, ...
    x = zero_tail(rnd(B, G * CIN, T, seed=60), ext, add, T)
    xv = GV.dense(x, G)
    w = rnd(G * Cout, CIN, K, seed=61, scale=0.05)
    wp = o.pack_weight(w, G, T=T, plain=False)
    assert getattr(wp, "nef_wino", 0) == 3
    table = torch.tensor(ext, dtype=torch.int32).to(DEV)
    dead = dead_mask(ext, add, PAD, T)
    assert bool(dead.any()) and not bool(dead.all())
    res_full = rnd(B, G * Cout, T, seed=62)
    res0 = zero_tail(res_full, ext, 0, T)                # ... and the identity residual's the table itself (block_fwd's conv2)
    res200 = zero_tail(res_full, ext, 200, T)            # a residual whose bound lies BEHIND some dead tiles: those do not qualify
    gate = GV.dense(rnd(B, G * Cout, T, seed=63), G)
    rows = (rnd(B, G, Cout, seed=64) + 0.3, G * Cout, Cout)
    bias = rnd(G * Cout, seed=65, scale=0.2)

    def run(name, slots=None, **kw):
        off, on = launch_pair(o, xv, wp, Cout, K, T, table, add, slots=slots, **kw)
        same(name, off, on)
        return off[0], on[0]

    y0, y1 = run("none")
    assert not bool(y1.view(B, G, Cout, T)[dead.expand(B, G, Cout, T)].any())
    for b in range(B):                                   # an extent-0 row (operand bound PAD): its output is zero from 2 PAD on
        for g_ in range(G):
            if ext[b][g_] == 0:
                assert not bool(y1.view(B, G, Cout, T)[b, g_, :, 2 * PAD:].any()), (b, g_)
    run("relu_dropout", relu=True, drop_p=0.2, drop_scale=1.25, seed=1234)
    run("res_promise", res=GV.dense(res0, G), res_live=0, relu=True)
    run("res_promise_scaled", res=GV.dense(res0, G), res_live=0, res_scale=rows, in_scale=(rnd(B, G, CIN, seed=66) + 0.3, G * CIN, CIN))
    # the same residual tensor, its promise not handed over, and one that is non-zero in the dead tiles: the result carries it
    run("res_no_promise_zero_tail", res=GV.dense(res0, G))
    _, y1 = run("res_no_promise", res=GV.dense(res_full, G))
    assert bool((y1.view(B, G, Cout, T) != 0)[dead.expand(B, G, Cout, T)].all())
    _, y1 = run("res_promise_behind", res=GV.dense(res200, G), res_live=200)
    part = dead & ~dead_mask(ext, 200, 0, T)             # dead for the operand, in front of the residual's bound
    assert bool(part.any()) and bool(y1.view(B, G, Cout, T)[part.expand(B, G, Cout, T)].any())
    _, y1 = run("bias", bias=bias)
    assert bool((y1.view(B, G, Cout, T) != 0)[dead.expand(B, G, Cout, T)].all())
    run("gate_pos", gate=gate, gate_scale=1.25)
    run("gate_rowscale", gate=gate, gate_scale=1.25, gate_rowscale=rows)
    y0, y1 = run("gate_neg", gate=gate, gate_scale=-1.25)
    d = dead.expand(B, G, Cout, T)
    assert bool(torch.signbit(y0.view(B, G, Cout, T)[d]).any())          # the full epilogue leaves -0.0 in the dead tiles ...
    assert not bool(torch.signbit(y1.view(B, G, Cout, T)[d]).any())      # ... the exit +0.0: it is what ran
    assert torch.equal(torch.signbit(y1.view(B, G, Cout, T)[~d]), torch.signbit(y0.view(B, G, Cout, T)[~d]))
    # the sign of a zero cannot leak into later bits: one more plain conv over both results
    w2 = rnd(G * 64, Cout, 3, seed=67, scale=0.05)
    wp2 = o.pack_weight(w2, G, T=T, plain=False)
    z0, z1 = (o.conv(GV.dense(y, G), wp2, 64, 3, x_scale=1.0) for y in (y0, y1))
    assert torch.equal(z1, z0) and bool(z0.any())
    # gate + stats_mode 1 (w_conv's channel-scale gradient): the launch keeps the full epilogue for its slot sums -- also under a
    # negative scale, where the sign tells
    slots = o.conv_stats_buffer(wp, B, G, Cout, T, torch.device(DEV))
    assert slots is not None
    run("gate_stats1", slots=slots, gate=gate, gate_rowscale=rows, stats=slots, stats_mode=1, res=GV.dense(res0, G), res_live=0)
    y0, y1 = run("gate_neg_stats1", slots=slots, gate=gate, gate_scale=-1.0, gate_rowscale=rows, stats=slots, stats_mode=1)
    assert torch.equal(torch.signbit(y1), torch.signbit(y0)) and bool(torch.signbit(y1.view(B, G, Cout, T)[d]).any())


def test_dead_tile_strided_output():
    """The output as one half of a wider tensor (block_bwd's `out`: batch and group strides that are not the dense ones): the exit
    writes its tile's rows and nothing else."""
    o = ops()
    from electrocardio_panorama_amd.ops import GV
    K, Cout, T = 3, 64, 602
    if not o.h2_ok(K, CIN, Cout, T):
        pytest.skip("split-fp16 convs switched off")
    ext = extents(T)
    x = zero_tail(rnd(B, G * CIN, T, seed=70), ext, 0, T)
    wp = o.pack_weight(rnd(G * Cout, CIN, K, seed=71, scale=0.05), G, T=T, plain=False)
    table = torch.tensor(ext, dtype=torch.int32).to(DEV)
    got = []
    for on in (False, True):
        o.LIVE = on
        try:
            wide = torch.full((B, G * 2 * Cout, T), 7.0, device=DEV)
            o.conv(GV.dense(x, G), wp, Cout, K, out=GV.half(wide, G, 1), live=(table, 0), relu=True)
            got.append(wide)
        finally:
            o.LIVE = True
    assert torch.equal(got[0], got[1])
    v = got[1].view(B, G, 2, Cout, T)
    assert bool((v[:, :, 0] == 7.0).all()) and not bool((v[:, :, 1] == 7.0).any())


# ------------------------------------------------------------------------------------------------ the stem's weight gradient
SB, SV, SL = 8, 3, 2400
STEM_E = [0, SL, 1000, 777, 1290, 2399, 60, 1]      # input extents, cycled over the 24 rows


@pytest.fixture(scope="module")
def stem_case():
    """Inputs and the fp64 weight gradient (autograd through max_pool(relu(conv))), computed once.  gy is random and non-zero
    everywhere: behind a row's extent it is the ReLU gate that has to kill it."""
    g = torch.Generator().manual_seed(80)
    x = torch.rand(SB, SV, SL, generator=g) + 0.05
    for r in range(SB * SV):
        x.view(-1, SL)[r, STEM_E[(r + r // 8) % len(STEM_E)]:] = 0.0
    w = (torch.rand(128 * SV, 1, 15, generator=g) * 2 - 1) * 0.3
    gy = torch.randn(SB, 128 * SV, SL // 4, generator=g)
    gy[gy == 0] = 1.0
    wr = w.double().requires_grad_(True)
    F.max_pool1d(F.relu(F.conv1d(x.double(), wr, None, 2, 7, 1, SV)), 3, 2, 1).backward(gy.double())
    return x.to(DEV), w.to(DEV), gy.to(DEV), wr.grad


def test_stem_bwd_weight_live_same_bits(stem_case):
    o = ops()
    x, w, gy, ref = stem_case
    table = o.live_extent(x)
    lv = table.cpu().flatten().tolist()
    assert 0 in lv and SL // 4 in lv and any(0 < e < SL // 4 and e % 16 for e in lv) and any(0 < e < 16 for e in lv), lv
    full = o.stem_bwd_weight(x, w, gy)
    cut = o.stem_bwd_weight(x, w, gy, live=table)
    assert torch.equal(cut, full)
    # the fp64 bar of tests/test_lengths_gpu.py for the kernel without a table: the whole tensor and each lead's block
    assert rel(full, ref) < GRAD_TOL
    for v in range(SV):
        blk = slice(128 * v, 128 * (v + 1))
        assert rel(cut[blk], ref[blk]) < GRAD_TOL, (v, rel(cut[blk], ref[blk]))
    # the switch: with ops.LIVE off the table is not handed on
    o.LIVE = False
    try:
        assert torch.equal(o.stem_bwd_weight(x, w, gy, live=torch.zeros_like(table)), full)
    finally:
        o.LIVE = True


def test_stem_bwd_weight_table_is_what_stops(stem_case):
    """The table is USED: a table of zeros walks no tile at all, one of 16 exactly the first tile of every row."""
    o = ops()
    x, w, gy, _ = stem_case
    x = x.clone()
    x[x == 0] = 0.5                                   # no zero tails: the table alone decides
    table = torch.zeros(SB, SV, dtype=torch.int32, device=DEV)
    assert not bool(o.stem_bwd_weight(x, w, gy, live=table).any())
    gy16 = gy.clone()
    gy16[:, :, 16:] = 0.0
    assert torch.equal(o.stem_bwd_weight(x, w, gy, live=table + 16), o.stem_bwd_weight(x, w, gy16))
    assert torch.equal(o.stem_bwd_weight(x, w, gy, live=table + 3), o.stem_bwd_weight(x, w, gy16))      # rounded up to a whole tile
