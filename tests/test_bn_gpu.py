"""Every BatchNorm kernel form of csrc/elementwise.hip (and the two helpers it inlines, the x2-upsampling adjoint and the
last conv's input gradient) against the fp64 reference of tests/bn_ref.py, at the smallest shapes that reach each branch.

Decision ties.  The kernels decide the ReLU on fmaf(x, a32, b32) > 0, the reference on x*a + b > 0 in fp64; one flipped
element moves ggamma / gbeta by far more than any tolerance.  The kernel's decision error is at most the relative error of
a and b (asserted <= 1e-6 here) plus one fma rounding, ~2.1e-6 of |x*a| + |b|, so every case first ASSERTS that no decision
of its inputs is closer to a tie than MARGIN = 2^-16 of |x*a| + |b| (seven times that) and then compares every element.
The seeds in SEEDS were searched on the CPU for that property (`python tests/test_bn_gpu.py` prints the table); a seed
that does not clear the screen fails its test.  Two families cannot clear it with continuous inputs at any seed and take
x from a 2^-7 lattice instead (gamma, beta and the gradients stay continuous, so x*a + b still rounds):
  - C = 64 with L >= 1028: 0.4 - 1.6 M decisions, ~10 expected within MARGIN of a tie; on the lattice only the lattice
    point nearest to each (pass, channel)'s tie point -b/a matters;
  - the conditioning sweep: at |mean|/std = 30 the two terms are ~30x the pre-activation, so MARGIN is 1e-3 of the
    pre-activation's own scale and ~25 of 83 k decisions would sit inside it.

Tolerances are the project's (test_batchnorm_train_three_passes): rel-L2 1e-6 for the statistics, FWD_TOL for the
forward, 1e-5 for gx / ggamma / gbeta, 2e-7 * max_c sum|gx| for the analytically zero channel sum of gx -- plus a
per-element bound max|d| <= 1e-5 * max|ref| on gx and the forward, so that one wrong edge column cannot hide in a norm.

Wrong-on-purpose edits of elementwise.hip tried against this file (each fails the tests named, none is committed):
`two = false` in bn_stats_partial -> the L = 8 statistics cases with Bp >= 9 and (1,17,5,1028); `t0 += 2048` in
bn_bwd_apply_rows -> every L = 4100 case; the last-vector condition of up2_adjoint4 never true, or its t4 == 0 line
dropped -> bn_relu_bwd_up at every L; oc_grad4's `lo` / `hi` guard off by one vector -> bn_relu_bwd_outconv at L >= 12;
`q += 512` in upsample2_bwd_rows -> upsample2 at Tin = 516, 1250; `b += 512` in bn_rows_reduce ->
pass_combine_fwd_stats (300,2,4); bn_stats_final / bn_bwd_final launched with one block -> the C = 65 cases; fold_bn
without `+ b` -> fold_bn; `>=` in gate4_kernel -> gate; the phase-major pair (o[0], o[1]) -> the phase-major cases;
`am = o[0] + o[1]` in bn_bwd_apply_combine3 -> the combine3 cases, slot-fed included."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref
from util import FWD_TOL, maxabs, rel, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN = 2.0 ** -16
STAT_TOL, GRAD_TOL5, ELEM_TOL, CHANSUM_TOL = 1e-6, 1e-5, 1e-5, 2e-7

# (P, Bp, C, L) -> seed whose inputs clear the tie screen (searched on the CPU, see the module docstring)
SEEDS = {
    (3, 1, 3, 2): 1000, (1, 9, 3, 257): 1000, (3, 4, 65, 250): 1014,
    (1, 1, 3, 8): 1000, (1, 8, 3, 8): 1000, (1, 9, 3, 8): 1000, (1, 16, 3, 8): 1000, (1, 17, 3, 8): 1000, (1, 24, 3, 8): 1000,
    (1, 17, 5, 1028): 1001, (3, 9, 3, 257): 1002, (3, 4, 16, 250): 1006, (3, 9, 65, 8): 1001, (3, 2, 3, 4100): 1008,
    (3, 2, 3, 8): 1000, (3, 2, 3, 12): 1000, (3, 2, 3, 1028): 1000, (3, 2, 3, 4): 1000,
    (3, 2, 64, 4): 1001, (3, 2, 64, 12): 1000, (3, 2, 64, 1028): 1001, (3, 2, 64, 4100): 1000,
    (3, 2, 3, 37): 1000, (3, 2, 3, 258): 1000, (3, 2, 3, 6): 1000,
    (3, 1, 64, 256): 1003,                                    # slot-fed backward: the BatchNorm input below the conv
    ("sweep", 0): 1000, ("sweep", 3): 1001, ("sweep", 30): 1003,
}
LATTICE = 128.0


def on_lattice(P, Bp, C, L):
    return C == 64 and L >= 1028


def ops():
    from electrocardio_panorama_amd import ops as o
    return o


def g(t):
    return t.float().to(DEV).contiguous()


def report(line):
    import conftest
    conftest.report(line)


_CASES = {}


def bn_case(P, Bp, C, L, seed=None):
    """Seeded fp32 inputs of one BatchNorm over P stacked passes and their fp64 statistics (computed once per shape)."""
    key = (P, Bp, C, L, seed)
    if key not in _CASES:
        s = SEEDS[(P, Bp, C, L)] if seed is None else seed
        x = rnd(P * Bp, C, L, seed=s) * 2 + 0.3
        if on_lattice(P, Bp, C, L):
            x = torch.round(x * LATTICE) / LATTICE
        gamma, beta = rnd(C, seed=s + 1) + 1.5, rnd(C, seed=s + 2)
        rm, rv = rnd(C, seed=s + 3) * 0.1, rnd(C, seed=s + 4).abs() + 0.5
        _CASES[key] = dict(P=P, Bp=Bp, C=C, L=L, seed=s, x=x, gamma=gamma, beta=beta, rm=rm, rv=rv,
                           ref=bn_ref.stats(x, gamma, beta, rm, rv, P))
    return _CASES[key]


def sweep_case(r, seed=None):
    """The conditioning sweep's inputs at (3, 9, 3, 1028): x = rnd * 0.577 + r/3 per channel (std 1/3, so |mean|/std = r),
    the sign of the offset alternating over the channels; x on the lattice (module docstring)."""
    key = ("sweep", r, seed)
    if key not in _CASES:
        P, Bp, C, L = 3, 9, 3, 1028
        s = SEEDS[("sweep", r)] if seed is None else seed
        sign = torch.tensor([1.0, -1.0, 1.0])
        x = torch.round(rnd(P * Bp, C, L, seed=s) * 0.577 * LATTICE) / LATTICE + (r / 3.0) * sign[None, :, None]
        gamma, beta = rnd(C, seed=s + 1) + 1.5, rnd(C, seed=s + 2)
        rm, rv = rnd(C, seed=s + 3) * 0.1, rnd(C, seed=s + 4).abs() + 0.5
        _CASES[key] = dict(P=P, Bp=Bp, C=C, L=L, seed=s, x=x, gamma=gamma, beta=beta, rm=rm, rv=rv,
                           ref=bn_ref.stats(x, gamma, beta, rm, rv, P))
    return _CASES[key]


def margin_of(c):
    return bn_ref.relu_margin(c["x"], c["ref"][2], c["ref"][3], c["P"])


def screen(c):
    """The tie screen: asserted, never skipped; nothing is excluded from the comparisons that follow."""
    m = margin_of(c)
    assert m >= MARGIN, f"seed {c['seed']} of {c['P'], c['Bp'], c['C'], c['L']}: closest ReLU decision at {m:.2e} < 2^-16"
    return m


def gpu_stats(o, c, tol=STAT_TOL, tols=None):
    """bn_train_stats on the device, checked against the fp64 reference; returns the device tensors and the errors."""
    rmd, rvd = g(c["rm"]), g(c["rv"])
    got = o.bn_train_stats(g(c["x"]), g(c["gamma"]), g(c["beta"]), rmd, rvd, c["P"])
    errs = [rel(q, r) for q, r in zip(list(got) + [rmd, rvd], c["ref"])]
    for name, e, t in zip(("mean", "invstd", "a", "b", "running_mean", "running_var"), errs, tols or [tol] * 6):
        assert e <= t, (name, e, t)
    return got, errs


def elem(got, ref):
    """max|got - ref| / max|ref|."""
    return maxabs(got, ref) / float(bn_ref.d(ref).abs().max())


def check_bwd(got, ref, tol=None):
    """(gx, ggamma, gbeta[, chan sum]) of a kernel against the reference's; returns the measured errors."""
    t = dict(gx=GRAD_TOL5, elem=ELEM_TOL, gg=GRAD_TOL5, gb=GRAD_TOL5)
    t.update(tol or {})
    e = dict(gx=rel(got[0], ref[0]), elem=elem(got[0], ref[0]), gg=rel(got[1], ref[1]), gb=rel(got[2], ref[2]))
    if len(got) > 3 and got[3] is not None:
        e["gs"] = maxabs(got[3], ref[3]) / float(ref[4].max())
        t["gs"] = CHANSUM_TOL
    for k in e:
        assert e[k] <= t[k], (k, e[k], t[k])
    return e


def bwd_ref(c, gy=None, g_of_act=None):
    """fp64 (gx, ggamma, gbeta, chan sum, per-channel sum|gx|) for the case's inputs."""
    fn = g_of_act if g_of_act is not None else (lambda act: bn_ref.d(gy))
    gx, gg, gb, gs, _ = bn_ref.bwd_g(fn, c["x"], c["gamma"], c["beta"], c["P"])
    return gx, gg, gb, gs, gx.abs().sum(dim=(0, 2))


def fmt(e):
    return " ".join(f"{k} {v:.1e}" for k, v in e.items())


# ------------------------------------------------------------------------------------------------ statistics and forward
STATS_SCALAR = [(3, 1, 3, 2), (1, 9, 3, 257), (3, 4, 65, 250)]
STATS_VEC = [(1, Bp, 3, 8) for Bp in (1, 8, 9, 16, 17, 24)] + [(1, 17, 5, 1028)]


@pytest.mark.parametrize("P,Bp,C,L", STATS_SCALAR + STATS_VEC)
def test_bn_train_stats_forward_eval(P, Bp, C, L):
    """bn_stats_partial (scalar branch for L % 4 != 0; 16-byte branch with its two-rows-in-flight pairing for every way Bp
    can fall against 2 * BN_SPLIT) + bn_stats_final (n = 2: unbiased factor 2; C = 65: second 64-thread block), then
    affine_relu_fwd on those statistics and bn_eval_affine + affine_relu_fwd on the updated running statistics."""
    o = ops()
    c = bn_case(P, Bp, C, L)
    m = screen(c)
    (mean, invstd, a, b), errs = gpu_stats(o, c)
    _, _, a64, b64, rm64, rv64 = c["ref"]
    y, yref = o.affine_relu_fwd(g(c["x"]), a, b, P), bn_ref.fwd(c["x"], a64, b64, P)
    e_fwd, e_el = rel(y, yref), elem(y, yref)
    assert e_fwd <= FWD_TOL and e_el <= ELEM_TOL
    # eval mode on the fp32 running statistics the reference left (the kernel's own inputs, not its outputs)
    rm32, rv32 = rm64.float(), rv64.float()
    a1, b1 = o.bn_eval_affine(g(c["gamma"]), g(c["beta"]), g(rm32), g(rv32))
    a1r, b1r = bn_ref.eval_affine(c["gamma"], c["beta"], rm32, rv32)
    assert a1.shape == (1, C) and rel(a1, a1r) <= STAT_TOL and rel(b1, b1r) <= STAT_TOL
    assert bn_ref.relu_margin(c["x"], a1r, b1r, 1) >= MARGIN
    ye, yeref = o.affine_relu_fwd(g(c["x"]), a1, b1, 1), bn_ref.fwd(c["x"], a1r, b1r, 1)
    assert rel(ye, yeref) <= FWD_TOL and elem(ye, yeref) <= ELEM_TOL
    report(f"bn_train_stats/affine_relu_fwd/bn_eval_affine {P, Bp, C, L}: stats {max(errs):.1e} fwd {e_fwd:.1e} elem {e_el:.1e} "
           f"eval {rel(ye, yeref):.1e} margin {m:.1e}")


def test_fold_bn():
    """fold_bn: w' = a*w and b' = a*bias + b element by element, and as a function: the fp64 conv with the folded weights
    equals eval-mode BatchNorm of the fp64 conv with the plain ones."""
    o = ops()
    Cout, Cin, K = 5, 7, 3
    w, bias = rnd(Cout, Cin, K, seed=900), rnd(Cout, seed=901)
    gamma, beta = rnd(Cout, seed=902) + 1.5, rnd(Cout, seed=903)
    rm, rv = rnd(Cout, seed=904) * 0.1, rnd(Cout, seed=905).abs() + 0.5
    a, b = o.bn_eval_affine(g(gamma), g(beta), g(rm), g(rv))
    wf, bf = o.fold_bn(g(w), g(bias), a, b)
    a64, b64 = bn_ref.eval_affine(gamma, beta, rm, rv)
    e_w, e_b = rel(wf, a64[0][:, None, None] * w.double()), rel(bf, a64[0] * bias.double() + b64[0])
    assert wf.shape == w.shape and bf.shape == bias.shape and e_w <= STAT_TOL and e_b <= STAT_TOL
    x = rnd(2, Cin, 19, seed=906).double()
    want = F.conv1d(x, w.double(), bias.double(), 1, 1) * a64[0][None, :, None] + b64[0][None, :, None]
    e_f = rel(F.conv1d(x, wf.double().cpu(), bf.double().cpu(), 1, 1), want)
    assert e_f <= STAT_TOL
    report(f"fold_bn Cout=5 inner=21: w {e_w:.1e} bias {e_b:.1e} folded conv vs eval-BN of the conv {e_f:.1e}")


# ------------------------------------------------------------------------------------------------ backward, plain
BWD_SCALAR = [(3, 9, 3, 257), (3, 4, 16, 250)]
BWD_ROWS = [(3, 9, 65, 8), (1, 17, 5, 1028), (3, 2, 3, 4100)]


@pytest.mark.parametrize("chan_sum", [True, False])
@pytest.mark.parametrize("P,Bp,C,L", BWD_SCALAR + BWD_ROWS)
def test_bn_relu_bwd(P, Bp, C, L, chan_sum):
    """bn_bwd_partial<0> (both branches) + bn_bwd_final + the wave-per-row bn_bwd_apply (L % 4 != 0) or bn_bwd_apply_rows<0>
    (L % 4 == 0; L = 4100 takes a second trip of its t0 loop), with and without the row sums."""
    o = ops()
    c = bn_case(P, Bp, C, L)
    m = screen(c)
    (mean, invstd, a, b), _ = gpu_stats(o, c)
    gy = rnd(P * Bp, C, L, seed=c["seed"] + 5)
    got = o.bn_relu_bwd(g(gy), g(c["x"]), g(c["gamma"]), mean, invstd, a, b, P, with_chan_sum=chan_sum)
    assert len(got) == (4 if chan_sum else 3)
    e = check_bwd(got, bwd_ref(c, gy))
    report(f"bn_relu_bwd {P, Bp, C, L} chan_sum={int(chan_sum)}: {fmt(e)} margin {m:.1e}")


@pytest.mark.parametrize("P,Bp,C,L", BWD_ROWS)
def test_bn_relu_bwd_phase_major(P, Bp, C, L):
    """bn_bwd_apply_rows<0> with the phase-major store: gx as [N, 2C, L/2], row 2c + p = positions p, p + 2, ..."""
    o = ops()
    c = bn_case(P, Bp, C, L)
    m = screen(c)
    (mean, invstd, a, b), _ = gpu_stats(o, c)
    gy = rnd(P * Bp, C, L, seed=c["seed"] + 5)
    got = o.bn_relu_bwd(g(gy), g(c["x"]), g(c["gamma"]), mean, invstd, a, b, P, with_chan_sum=True, phase_major=True)
    ref = bwd_ref(c, gy)
    assert got[0].shape == (P * Bp, 2 * C, L // 2)
    e = check_bwd(got, (bn_ref.phase_major(ref[0]),) + ref[1:])
    report(f"bn_relu_bwd phase_major {P, Bp, C, L}: {fmt(e)} margin {m:.1e}")


# ------------------------------------------------------------------------------------------------ backward, fused producers
@pytest.mark.parametrize("L", [8, 12, 1028, 4100])
def test_bn_relu_bwd_up(L):
    """bn_bwd_partial<2> + bn_bwd_apply_rows<2>: the x2-upsampling adjoint rebuilt from the [N, C, 2L] gradient (up2_adjoint4:
    the clamped taps at t4 == 0 and at the last vector of a row; L = 8 and 12 have one and no interior vector)."""
    o = ops()
    P, Bp, C = 3, 2, 3
    c = bn_case(P, Bp, C, L)
    m = screen(c)
    (mean, invstd, a, b), _ = gpu_stats(o, c)
    gu = rnd(P * Bp, C, 2 * L, seed=c["seed"] + 6)
    got = o.bn_relu_bwd_up(g(gu), g(c["x"]), mean, invstd, a, b, P)
    e = check_bwd(got, bwd_ref(c, bn_ref.upsample2_adjoint(gu)))
    report(f"bn_relu_bwd_up {P, Bp, C, L}: {fmt(e)} margin {m:.1e}")


@pytest.mark.parametrize("C", [3, 64])
@pytest.mark.parametrize("L", [4, 12, 1028, 4100])
def test_bn_relu_bwd_outconv(L, C):
    """outconv_go + bn_bwd_partial<1> + bn_bwd_apply_rows<1>: the last conv's input gradient rebuilt from its go row
    (oc_grad4: zero padding at t4 == 0 and at the last vector).  `out` is outconv_fwd(pro=...)'s, checked first."""
    o = ops()
    P, Bp = 3, 2
    c = bn_case(P, Bp, C, L)
    m = screen(c)
    (mean, invstd, a, b), _ = gpu_stats(o, c)
    w, bias = rnd(1, C, 3, seed=c["seed"] + 7, scale=0.2), rnd(1, seed=c["seed"] + 8)
    gout = rnd(P * Bp, 1, L, seed=c["seed"] + 9)
    out = o.outconv_fwd(g(c["x"]), g(w), g(bias), pro=(a, b, Bp))
    act64 = bn_ref.fwd(c["x"], c["ref"][2], c["ref"][3], P)
    e_out = rel(out, bn_ref.outconv(act64, w, bias))
    assert e_out <= STAT_TOL and elem(out, bn_ref.outconv(act64, w, bias)) <= ELEM_TOL
    got = o.bn_relu_bwd_outconv(g(gout), out, g(w), g(c["x"]), mean, invstd, a, b, P)
    e = check_bwd(got, bwd_ref(c, g_of_act=lambda act: bn_ref.outconv_adjoint(gout, act, w, bias)))
    report(f"bn_relu_bwd_outconv {P, Bp, C, L}: out {e_out:.1e} {fmt(e)} margin {m:.1e}")


@pytest.mark.parametrize("L,phase_major", [(37, False), (258, False), (6, True), (258, True)])
def test_bn_relu_bwd_combine3(L, phase_major):
    """bn_bwd_apply_combine3: the three passes' gx folded through the pass adjoint (A[mean] = g0 + g2, A[pick] = g1,
    B[mean] = g0 + g1, B[pick] = g2), plain and phase-major; L = 258 takes a second thread trip."""
    o = ops()
    P, Bp, C = 3, 2, 3
    c = bn_case(P, Bp, C, L)
    m = screen(c)
    (mean, invstd, a, b), _ = gpu_stats(o, c)
    gy = rnd(P * Bp, C, L, seed=c["seed"] + 5)
    got = o.bn_relu_bwd_combine3(g(gy), g(c["x"]), mean, invstd, a, b, phase_major=phase_major)
    ref = bwd_ref(c, gy)
    want = bn_ref.combine3(ref[0])
    if phase_major:
        want = bn_ref.phase_major(want)
    assert got[0].shape == want.shape
    e = check_bwd(got, (want,) + ref[1:])
    report(f"bn_relu_bwd_combine3 {Bp, C, L} phase_major={int(phase_major)}: {fmt(e)} margin {m:.1e}")


@pytest.mark.parametrize("B,C,L", [(3, 8, 37), (300, 2, 4)])
def test_pass_combine_fwd_stats(B, C, L):
    """pass_combine_fwd_stats_kernel + bn_rows_reduce (B = 300: its loop past 256 rows) + bn_stats_final(nsplit = 1): c1 is
    the fp32 sum (a + b) + bias exactly, its statistics are those of the fp64 reference on that c1."""
    o = ops()
    P2, bias = rnd(2 * B, 2 * C, L, seed=920) * 2 + 0.3, rnd(C, seed=921)
    gamma, beta = rnd(C, seed=922) + 1.5, rnd(C, seed=923)
    rm, rv = rnd(C, seed=924) * 0.1, rnd(C, seed=925).abs() + 0.5
    rmd, rvd = g(rm), g(rv)
    c1, mean, invstd, a, b = o.pass_combine_fwd_stats(g(P2), g(bias), B, g(gamma), g(beta), rmd, rvd)
    am, bm, ap, bp = P2[:B, :C], P2[:B, C:], P2[B:, :C], P2[B:, C:]
    c1_32 = torch.cat([am + bm, ap + bm, am + bp], 0) + bias[None, :, None]
    assert torch.equal(c1.cpu(), c1_32) and rel(c1, bn_ref.pass_combine_fwd(P2, bias, B)) <= STAT_TOL
    assert torch.equal(o.pass_combine_fwd(g(P2), g(bias), B), c1)
    ref = bn_ref.stats(c1_32, gamma, beta, rm, rv, 3)
    errs = [rel(q, r) for q, r in zip((mean, invstd, a, b, rmd, rvd), ref)]
    assert max(errs) <= STAT_TOL, errs
    report(f"pass_combine_fwd_stats {B, C, L}: c1 exact, stats {max(errs):.1e}")


# ------------------------------------------------------------------------------------------------ slot-fed forms
@pytest.fixture(params=[True, False], ids=["h2", "fp32"])
def h2(request):
    """The slot sums come from a conv epilogue: the split-fp16 kernel's (ops.H2) or the F(4,3) kernel's."""
    o = ops()
    saved, hint = o.H2, o.BATCH_HINT
    o.H2, o.BATCH_HINT = request.param, None
    yield request.param
    o.H2, o.BATCH_HINT = saved, hint


def _need_f43(o, h2):
    if not h2 and o.WINO_FWD != 2:
        pytest.skip("F(4,3) switched off (NEF_WINOGRAD): no fp32 kernel leaves slot sums")


SLOT_SHAPE = (3, 64, 64, 514)      # B, Cin, Cout, T: test_conv_epilogue_bn_slot_sums's smallest case (fewest multiply-adds)


def _slot_inputs(seed=180):
    B, Cin, Cout, T = SLOT_SHAPE
    return (rnd(B, Cin, T, seed=seed), rnd(Cout, Cin, 3, seed=seed + 1, scale=0.05), rnd(3, Cin, seed=seed + 7) * 0.5 + 1.0,
            rnd(3, Cin, seed=seed + 8) * 0.2)


def _slot_conv(o, bias):
    """test_conv_epilogue_bn_slot_sums's setup at its smallest shape: a K = 3 conv with the BatchNorm-ReLU prologue whose
    epilogue leaves the slot sums; returns the conv output (device) and the slots."""
    from electrocardio_panorama_amd.ops import GV
    B, Cin, Cout, T = SLOT_SHAPE
    x, w, pa, pb = (g(t) for t in _slot_inputs())
    wp = o.pack_weight(w, 1, T=T, f4=True)
    slots = o.conv_stats_buffer(wp, B, 1, Cout, T, x.device)
    assert slots is not None and slots[0].shape == (Cout, B * slots[1], 2)
    slots[0].fill_(float("nan"))                     # every slot must be written
    y = o.conv(GV.dense(x, 1), wp, Cout, 3, bias=g(bias), pro=(1, pa, pb, B // 3), stats=slots)
    return y, slots, (B, Cout, T)


def _slot_conv_moments():
    """Per-channel mean and standard deviation of that conv's output without its bias, in fp64 on the CPU."""
    x, w, pa, pb = _slot_inputs()
    y = F.conv1d(bn_ref.fwd(x, pa, pb, 3), w.double(), None, 1, 1)
    return y.mean(dim=(0, 2)), y.std(dim=(0, 2))


def test_bn_stats_from_slots(h2):
    """bn_slots_stats_fused on the conv epilogue's slot sums against the fp64 statistics of the tensor the conv wrote."""
    o = ops()
    _need_f43(o, h2)
    Cout = 64
    y, slots, (B, _, T) = _slot_conv(o, rnd(Cout, seed=182))
    gamma, beta = rnd(Cout, seed=183) + 1.2, rnd(Cout, seed=184, scale=0.3)
    rm, rv = rnd(Cout, seed=185) * 0.1, rnd(Cout, seed=186).abs() + 0.5
    rmd, rvd = g(rm), g(rv)
    got = o.bn_stats_from_slots(slots, g(gamma), g(beta), rmd, rvd, 3, B, T)
    ref = bn_ref.stats(y, gamma, beta, rm, rv, 3)
    errs = [rel(q, r) for q, r in zip(list(got) + [rmd, rvd], ref)]
    assert max(errs) <= STAT_TOL, errs
    report(f"bn_stats_from_slots {B, Cout, T} {'split-fp16' if h2 else 'F(4,3)'} conv: stats {max(errs):.1e}")


def test_bn_relu_bwd_slot_fed(h2):
    """bn_slots_bwd_fused + the apply kernels fed by the slot sums a backward-data launch left (the setup of
    test_conv_epilogue_bn_backward_slot_sums at its smallest shape), against the fp64 reference on the gradient the conv
    wrote: bn_relu_bwd(slots=...) and bn_relu_bwd_combine3(slots=...)."""
    o = ops()
    _need_f43(o, h2)
    from electrocardio_panorama_amd.ops import GV
    B, Cin, Cout, T = 3, 128, 64, 256
    c = bn_case(3, B // 3, Cout, T)                        # the lower layer's conv output (BatchNorm input)
    m = screen(c)
    gc = g(rnd(B, Cin, T, seed=190))                       # gradient at the upper layer's conv output
    w = g(rnd(Cin, Cout, 3, seed=191, scale=0.05))         # upper conv weight
    c_below, gamma = g(c["x"]), g(c["gamma"])
    (mean, invstd, a, b), _ = gpu_stats(o, c)
    wpf = o.pack_weight(w, 1, flip=True, T=T, f4=True)
    slots = o.conv_stats_buffer(wpf, B, 1, Cout, T, gc.device)
    assert slots is not None
    slots[0].fill_(float("nan"))
    gv = o.conv(GV.dense(gc, 1), wpf, Cout, 3, role="conv_bwd_data", bnb=(c_below, mean, invstd, a, b, B // 3, slots))
    ref = bwd_ref(c, gv)
    e = check_bwd(o.bn_relu_bwd(gv, c_below, gamma, mean, invstd, a, b, 3, with_chan_sum=True, slots=slots), ref)
    e3 = check_bwd(o.bn_relu_bwd_combine3(gv, c_below, mean, invstd, a, b, slots=slots), (bn_ref.combine3(ref[0]),) + ref[1:])
    report(f"slot-fed bn_relu_bwd {B, Cout, T} {'split-fp16' if h2 else 'F(4,3)'} conv: {fmt(e)} | combine3 {fmt(e3)} margin {m:.1e}")


# ------------------------------------------------------------------------------------------------ the two inlined helpers
@pytest.mark.parametrize("Tin", [4, 6, 65, 516, 1250])
def test_upsample2(Tin):
    """upsample2_fwd and upsample2_bwd (upsample2_bwd_rows for even Tin >= 4: Tin = 516 and 1250 take a second q trip; the
    shuffle kernel for Tin = 65) against fp64 F.interpolate and its adjoint."""
    o = ops()
    x, gy = rnd(2, 3, Tin, seed=930), rnd(2, 3, 2 * Tin, seed=931)
    y, yref = o.upsample2_fwd(g(x)), bn_ref.upsample2(x)
    gx, gxref = o.upsample2_bwd(g(gy)), bn_ref.upsample2_adjoint(gy)
    e = dict(fwd=rel(y, yref), fwd_elem=elem(y, yref), bwd=rel(gx, gxref), bwd_elem=elem(gx, gxref))
    assert e["fwd"] <= STAT_TOL and e["bwd"] <= STAT_TOL and e["fwd_elem"] <= ELEM_TOL and e["bwd_elem"] <= ELEM_TOL
    report(f"upsample2 Tin={Tin}: {fmt(e)}")


def test_gate():
    """gate4_kernel (n % 4 == 0, 16-byte aligned) and gate_kernel (the same data one float into the buffers): both are
    where(ref > 0, g * s, 0) exactly, zeros of either sign in `ref` included."""
    o = ops()
    n, s = 4096, 1.25
    gbuf, rbuf = rnd(n + 4, seed=940), rnd(n + 4, seed=941)
    rbuf[5], rbuf[6], rbuf[n - 1], rbuf[n] = 0.0, -0.0, 0.0, -0.0
    gd, rd = g(gbuf), g(rbuf)
    assert gd.data_ptr() % 16 == 0 and rd.data_ptr() % 16 == 0
    for off in (0, 1):
        gv, rv = gd[off:off + n], rd[off:off + n]
        want = torch.where(rbuf[off:off + n] > 0, gbuf[off:off + n] * s, torch.zeros(n))
        assert torch.equal(o.gate(gv, rv, s).cpu(), want), off
    report("gate n=4096: gate4_kernel (aligned) and gate_kernel (offset by one float) exact")


# ------------------------------------------------------------------------------------------------ conditioning
def _torch32(c, gy):
    """torch's own fp32 CPU BatchNorm + autograd on the case's inputs, pass by pass: the statistics, the forward and the
    gradients whose distance from the fp64 reference is the yardstick of the offset cases."""
    P, Bp = c["P"], c["Bp"]
    xr, gr, br = (c[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    rm, rv = c["rm"].clone(), c["rv"].clone()
    ys, ms, iss = [], [], []
    for p in range(P):
        y, m, i = torch.native_batch_norm(xr[p * Bp:(p + 1) * Bp], gr, br, rm, rv, True, 0.1, 1e-5)
        ys.append(F.relu(y)), ms.append(m.detach()), iss.append(i.detach())
    y = torch.cat(ys, 0)
    y.backward(gy)
    mean, invstd = torch.stack(ms), torch.stack(iss)
    a = c["gamma"][None, :] * invstd
    return (mean, invstd, a, c["beta"][None, :] - mean * a, rm, rv), y.detach(), (xr.grad, gr.grad, br.grad)


@pytest.mark.parametrize("r", [0, 3, 30])
def test_conditioning_fp64_sum_path(r):
    """bn_train_stats + bn_relu_bwd at |mean|/std = r: the kernels sum in fp64 from the first element, so their error should
    stay flat in r.  Bound per quantity: max(project tolerance, 4 x the distance of torch's fp32 CPU BatchNorm / autograd
    from the fp64 reference on the same inputs) -- the kernels have no reason to be worse than torch-fp32, but do round the
    mean to fp32 once more."""
    o = ops()
    c = sweep_case(r)
    P, Bp, C, L = c["P"], c["Bp"], c["C"], c["L"]
    m = screen(c)
    gy = rnd(P * Bp, C, L, seed=c["seed"] + 5)
    ref = bwd_ref(c, gy)
    st32, y32, gr32 = _torch32(c, gy)
    yref = bn_ref.fwd(c["x"], c["ref"][2], c["ref"][3], P)
    d_stats = [rel(q, w) for q, w in zip(st32, c["ref"])]
    d32 = dict(fwd=rel(y32, yref), fwd_elem=elem(y32, yref), gx=rel(gr32[0], ref[0]), elem=elem(gr32[0], ref[0]),
               gg=rel(gr32[1], ref[1]), gb=rel(gr32[2], ref[2]))
    (mean, invstd, a, b), errs = gpu_stats(o, c, tols=[max(STAT_TOL, 4 * q) for q in d_stats])
    y = o.affine_relu_fwd(g(c["x"]), a, b, P)
    e_fwd, e_el = rel(y, yref), elem(y, yref)
    assert e_fwd <= max(FWD_TOL, 4 * d32["fwd"]) and e_el <= max(ELEM_TOL, 4 * d32["fwd_elem"])
    got = o.bn_relu_bwd(g(gy), g(c["x"]), g(c["gamma"]), mean, invstd, a, b, P, with_chan_sum=True)
    e = check_bwd(got, ref, tol={k: max(t, 4 * d32[k]) for k, t in
                                 (("gx", GRAD_TOL5), ("elem", ELEM_TOL), ("gg", GRAD_TOL5), ("gb", GRAD_TOL5))})
    report(f"conditioning, fp64-sum path r={r}: stats {max(errs):.1e} (torch fp32 {max(d_stats):.1e}) fwd {e_fwd:.1e} "
           f"({d32['fwd']:.1e}) {fmt(e)} (torch fp32 gx {d32['gx']:.1e} elem {d32['elem']:.1e} gg {d32['gg']:.1e} "
           f"gb {d32['gb']:.1e}) margin {m:.1e}")


@pytest.mark.parametrize("r", [0, 3, 30])
def test_conditioning_slot_path(r, h2):
    """bn_stats_from_slots on a conv output whose bias puts every channel at |mean|/std ~ r.  The slot path forms
    E[y^2] - m^2 from fp32 sums: a slot is a depth-7 fp32 tree over 128 columns plus one rounding for the square, so
    |d s2|/s2 <= 8u and |d m| <= 7u sqrt(E[y^2]) (u = 2^-24), hence |d var|/var <= 22 * 2^-24 * (1 + r^2) with r the
    (pass, channel)'s own ratio in the fp64 reference.  Asserted for the variance; half of it plus 2^-23 for invstd."""
    o = ops()
    _need_f43(o, h2)
    Cout, eps = 64, 1e-5
    sign = torch.tensor([1.0, -1.0]).repeat(Cout // 2)
    mu, sd = _slot_conv_moments()
    bias = (r * sd * sign - mu).float()      # (the three passes differ a little: each keeps its own ratio in the bound)
    y, slots, (B, _, T) = _slot_conv(o, bias)
    gamma, beta = rnd(Cout, seed=183) + 1.2, rnd(Cout, seed=184, scale=0.3)
    mean, invstd, a, b = o.bn_stats_from_slots(slots, g(gamma), g(beta), g(torch.zeros(Cout)), g(torch.ones(Cout)), 3, B, T)
    m64, is64, _, _, _, _ = bn_ref.stats(y, gamma, beta, torch.zeros(Cout), torch.ones(Cout), 3)
    var64 = 1.0 / is64 ** 2 - eps
    ratio = m64.abs() / var64.sqrt()
    bound = 22 * 2.0 ** -24 * (1 + ratio ** 2)
    var = 1.0 / invstd.double().cpu() ** 2 - eps
    e_is = ((invstd.double().cpu() - is64).abs() / is64)
    # the variance is not an output: it is recovered from the fp32 invstd, whose own rounding is charged to the kernel
    e_var = ((var - var64).abs() / var64)
    y32 = y.cpu()
    is32 = torch.stack([torch.native_batch_norm(y32[p * (B // 3):(p + 1) * (B // 3)], None, None, None, None, True, 0.1, eps)[2]
                        for p in range(3)])
    d32 = float(((is32.double() - is64).abs() / is64).max())
    assert bool((e_is <= bound / 2 + 2.0 ** -23).all()), (float(e_is.max()), float(bound.max()))
    assert bool((e_var <= bound).all()), (float(e_var.max()), float(bound.max()))
    report(f"conditioning, slot path r={r} ({'split-fp16' if h2 else 'F(4,3)'} conv, measured ratio {float(ratio.min()):.1f}..{float(ratio.max()):.1f}): "
           f"var {float(e_var.max()):.1e} invstd {float(e_is.max()):.1e} (bound on var {float(bound.max()):.1e}; "
           f"torch fp32 invstd {d32:.1e}) mean {rel(mean, m64):.1e}")


def _search(key, start=1000, tries=400):
    for s in range(start, start + tries):
        c = sweep_case(key[1], seed=s) if key[0] == "sweep" else bn_case(*key, seed=s)
        ok = margin_of(c) >= MARGIN
        if ok and key[0] != "sweep":       # the eval-mode forward of the statistics cases is screened too
            a1, b1 = bn_ref.eval_affine(c["gamma"], c["beta"], c["ref"][4].float(), c["ref"][5].float())
            ok = bn_ref.relu_margin(c["x"], a1, b1, 1) >= MARGIN
        _CASES.clear()
        if ok:
            return s
    raise SystemExit(f"no seed for {key}")


if __name__ == "__main__":      # CPU only: print a SEEDS table whose inputs clear the tie screen
    for k in SEEDS:
        print(f"    {k}: {_search(k)},")
