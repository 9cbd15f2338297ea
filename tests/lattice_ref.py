"""Exact-arithmetic references for the conv kernels: operands on a small dyadic lattice, everything in plain torch on the CPU.

Every operand is drawn from a short list of dyadic values with at most a few significant bits (`lat`), so every product is exact
in fp32 (and in fp16 x fp16 -> fp32), and every partial sum of a dot product -- in ANY order -- is an integer multiple of one power
of two (`grid`) that stays far below 2^24 of them (`units`).  A kernel that multiplies the right pairs and adds them up in fp32 then
reproduces the fp64 result bit for bit; one missing, doubled or foreign product moves an element by at least `step`.  The functions
here take the dtype of their operands, so the same restatement runs in fp64 (the reference) and in fp32 (torch's own CPU op, which
tests/test_lattice_ref_cpu.py holds to it).  The preconditions are computed from the reference alone and asserted by `precheck`
wherever a case is built -- never skipped.

The case tables of tests/test_exact_gpu.py live here too, so that the CPU file can walk them without a GPU.
"""
import torch
import torch.nn.functional as F

X_VALS = (-2.0, -1.0, 1.0, 2.0)                     # activations and gradients
W_VALS = (-1.0, -0.5, 0.5, 1.0)                     # weights
R_VALS = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)          # bias, residual and in_scale rows
PA_VALS = (0.5, 1.0, 2.0)                           # BatchNorm-affine prologue: slope
PB_VALS = (-1.0, 0.0, 1.0)                          # ... and offset
DROP_SCALE = 1.25                                   # gate, dropout and residual scales are dyadic too
GATE_SCALE = 1.25
UNIT_LIMIT = 2 ** 24


def lat(shape, values=X_VALS, seed=0):
    """A float64 tensor of `shape` drawn uniformly from `values`."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(len(values), tuple(shape), generator=g)
    return torch.tensor(values, dtype=torch.float64)[idx]


def keep_mask(shape, seed):
    """A replayed dropout mask: uint8, ~80 % ones."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(tuple(shape), generator=g) > 0.2).to(torch.uint8)


def grid_of(*tensors):
    """The largest power of two that divides every entry of the tensors (1.0 if all are zero)."""
    v = torch.cat([t.detach().double().reshape(-1) for t in tensors])
    v = v[v != 0].abs()
    if v.numel() == 0:
        return 1.0
    assert bool(torch.isfinite(v).all())
    m, e = torch.frexp(v)                                # v = m * 2^e, 0.5 <= m < 1
    mi = (m * 2.0 ** 53).to(torch.int64)                 # the 53-bit mantissa as an integer
    low = (mi & -mi).double().log2()                     # its lowest set bit
    return 2.0 ** float((e.double() - 53 + low).min())


def fits_half(t):
    """Every entry survives a round trip through fp16."""
    t = t.detach().double()
    return bool((t.half().double() == t).all())


def min_nonzero(t):
    v = t.detach().double().abs().reshape(-1)
    v = v[v != 0]
    return float(v.min()) if v.numel() else 0.0


def precheck(ref, term_sum, term_grid, operands, step=None):
    """The preconditions of an exact comparison, from the reference alone:
    grid  = the largest power of two that divides every reference output,
    units = max sum |terms| / min(grid, grid of the terms) < 2^24  (every partial sum, in any order, is then an exact fp32 number),
    every operand, as the kernel multiplies it, survives fp16.  Returns (grid, units)."""
    grid = grid_of(ref)
    fine = min(grid, float(term_grid))
    units = float(term_sum) / fine
    assert units < UNIT_LIMIT, (units, grid, term_grid)
    assert float(ref.detach().abs().max()) / fine < UNIT_LIMIT
    for op in operands:
        assert fits_half(op), "an operand leaves the fp16 lattice"
    if step is not None:
        assert step >= fine, (step, fine)
    return grid, units


# ------------------------------------------------------------------------------------------------ the operations, any dtype
def launch_weight(w, G, flip):
    """The weight [G*Cout, Cin, K] of the FORWARD conv a launch computes: w itself, or -- flip, the backward-data launch of
    y = conv1d(x, w) -- its transpose within each group with the taps reversed."""
    if not flip:
        return w
    Cog, Cig, K = w.shape[0] // G, w.shape[1], w.shape[2]
    return w.view(G, Cog, Cig, K).transpose(1, 2).flip(3).reshape(G * Cig, Cog, K).contiguous()


def conv(x, w, G, bias=None):
    return F.conv1d(x, w, bias, 1, w.shape[2] // 2, 1, G)


def conv_bwd_data(gy, w, G):
    """Gradient of conv(x, w, G) wrt x, from torch's own adjoint (not through launch_weight)."""
    B, T = gy.shape[0], gy.shape[2]
    return torch.nn.grad.conv1d_input((B, G * w.shape[1], T), w, gy, padding=w.shape[2] // 2, groups=G)


def conv_bwd_weight(x, gy, G, K):
    Cog, Cig = gy.shape[1] // G, x.shape[1] // G
    return torch.nn.grad.conv1d_weight(x, (G * Cog, Cig, K), gy, padding=K // 2, groups=G)


def upsample2(x):
    return F.interpolate(x, scale_factor=2, mode="linear", align_corners=False)


def upsample2_bwd(gy):
    """The adjoint of upsample2, written out: gy [.., 2T] -> gx [.., T]."""
    T = gy.shape[-1] // 2
    ev, od = gy[..., 0::2], gy[..., 1::2]                # y[2m] = .25 x[m-1] + .75 x[m],  y[2m+1] = .75 x[m] + .25 x[m+1] (clamped)
    gx = 0.75 * (ev + od)
    gx[..., 1:] += 0.25 * od[..., :-1]
    gx[..., :-1] += 0.25 * ev[..., 1:]
    gx[..., 0] += 0.25 * ev[..., 0]
    gx[..., T - 1] += 0.25 * od[..., T - 1]
    return gx


def prologue(x, mode, a=None, b=None, Bp=1):
    """The input prologue of a conv launch: bit0 BatchNorm affine + ReLU with a / b [P, C] (pass p = sample // Bp), bit1 x2 linear
    upsampling."""
    if mode & 1:
        x = F.relu(x * a.repeat_interleave(Bp, 0)[:, :, None] + b.repeat_interleave(Bp, 0)[:, :, None])
    if mode & 2:
        x = upsample2(x)
    return x


def epilogue(y, res=None, relu=False, mask=None, drop_scale=1.0, gate=None, gate_scale=1.0, res_scale=None, gate_rowscale=None):
    """conv()'s epilogue after the bias: + res * res_scale, ReLU, replayed dropout, gate.  Returns (output, the output before the gate)."""
    if res is not None:
        y = y + (res if res_scale is None else res * res_scale[:, :, None])
    if relu:
        y = F.relu(y)
    if mask is not None:
        y = y * mask.to(y.dtype) * drop_scale
    pre = y
    if gate is not None:
        s = gate_scale if gate_rowscale is None else gate_scale * gate_rowscale[:, :, None]
        y = torch.where(gate > 0, y * s, torch.zeros_like(y))
    return y, pre


def slot_sums(y, width=128):
    """Per (sample, channel, slot of `width` columns): (sum y, sum y^2) -> [B, C, nslot, 2]."""
    B, C, T = y.shape
    n = (T + width - 1) // width
    yp = F.pad(y, (0, n * width - T)).view(B, C, n, width)
    return torch.stack([yp.sum(3), (yp * yp).sum(3)], 3)


def bn_backward_sums(g, x, mean, invstd, a, b, Bp, width=128):
    """Per (sample, channel, slot): (sum g m, sum g m xhat) with m = [a x + b > 0], xhat = (x - mean) invstd; the statistics are
    [P, C], pass p = sample // Bp."""
    e = lambda t: t.repeat_interleave(Bp, 0)[:, :, None]
    m = (x * e(a) + e(b) > 0).to(g.dtype)
    xh = (x - e(mean)) * e(invstd)
    B, C, T = g.shape
    n = (T + width - 1) // width
    pad = lambda t: F.pad(t, (0, n * width - T)).view(B, C, n, width)
    return torch.stack([pad(g * m).sum(3), pad(g * m * xh).sum(3)], 3)


def stem(x, w):
    V = x.shape[1]
    return F.max_pool1d(F.relu(F.conv1d(x, w, None, 2, 7, 1, V)), 3, 2, 1)


def stem_bwd_weight(x, w, gy):
    wr = w.clone().requires_grad_(True)
    stem(x, wr).backward(gy)
    return wr.grad


def convt2(x, w, bias, G):
    return F.conv_transpose1d(x, w, bias, 2, 0, 0, G)


def convt2_grads(x, w, bias, gy, G):
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, bias))
    convt2(xr, wr, br, G).backward(gy)
    return xr.grad, wr.grad, br.grad


def lead_mean(z1, z2r, V):
    B, _, T = z1.shape
    return torch.cat([z1.view(B, V, 128, T).mean(1), z2r.view(B, V, 128, T).mean(1)], 1)


def mix(latent, z1, z2r, q, V, c1, c2):
    z1m, z2m = latent[:, :128], latent[:, 128:]
    qq = q[:, :, None]
    return torch.cat([qq * latent, qq * torch.cat([z1[:, 128 * c1:128 * (c1 + 1)], z2m], 1),
                      qq * torch.cat([z1m, z2r[:, 128 * c2:128 * (c2 + 1)]], 1)], 0)


# ------------------------------------------------------------------------------------------------ sums of |terms|
def conv_terms(x, w, G):
    """max over the outputs of sum |w| |x|, and the grid of the products."""
    return float(conv(x.abs(), w.abs(), G).max()), grid_of(x) * grid_of(w)


def wgrad_terms(x, gy, G, K):
    return float(conv_bwd_weight(x.abs(), gy.abs(), G, K).max()), grid_of(x) * grid_of(gy)


def wino23_terms(x, w, G):
    """Winograd F(2,3) of a K = 3 conv, as the kernel multiplies: per output pair (2j, 2j+1) and plane, sum over the input channels
    of |B^T d| |G g|, with d = x[2j-1 .. 2j+2] (zero padded), B^T d = (d0 - d2, d1 + d2, d2 - d1, d1 - d3) and
    G g = (g0, ((g0 + g1) + g2) / 2, ((g0 - g1) + g2) / 2, g2); y[2j] = M0 + M1 + M2, y[2j+1] = M1 - M2 - M3.  Returns (the largest
    sum of |terms| of an output, the grid of the terms, the transformed operands)."""
    B, C, T = x.shape
    assert T % 2 == 0 and w.shape[2] == 3
    Cin, Cout = C // G, w.shape[0] // G
    xp = F.pad(x, (1, 1)).view(B, G, Cin, T + 2)
    d = [xp[..., i:i + T:2] for i in range(4)]                                  # [B, G, Cin, T/2] each
    v = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    g0, g1, g2 = (w.view(G, Cout, Cin, 3)[..., i] for i in range(3))
    u = [g0, ((g0 + g1) + g2) * 0.5, ((g0 - g1) + g2) * 0.5, g2]
    A = [torch.einsum("goc,bgcj->bgoj", ui.abs(), vi.abs()) for ui, vi in zip(u, v)]
    worst = max(float((A[0] + A[1] + A[2]).max()), float((A[1] + A[2] + A[3]).max()))
    return worst, grid_of(*u) * grid_of(*v), u + v


# ------------------------------------------------------------------------------------------------ case builders
def conv_launch(K, G, Cin, Cout, T, B, flip=False, seed=0, tail_zeros=0, x_mul=1.0, spike=None, wino23=False):
    """One forward / backward-data launch on the lattice.  `x` [B, G*Cin, T] is the launch's input (the gradient when `flip`), `w` the
    layer's weight in torch layout ([G*Cout, Cin, K]; flip: [G*Cin, Cout, K]).  `tail_zeros`: the last columns of every input row are
    exact zeros; `x_mul`: a power of two on the whole input; `spike` = (flat index, factor): one element times a power of two."""
    x = lat((B, G * Cin, T), X_VALS, seed + 1) * x_mul
    if tail_zeros:
        x[:, :, T - tail_zeros:] = 0.0
    if spike is not None:
        x.view(-1)[spike[0] % x.numel()] *= spike[1]
    w = lat((G * Cin, Cout, K) if flip else (G * Cout, Cin, K), W_VALS, seed + 2)
    ref = conv_bwd_data(x, w, G) if flip else conv(x, w, G)
    weff = launch_weight(w, G, flip)
    if flip:
        assert torch.equal(ref, conv(x, weff, G))       # the adjoint restated as a forward conv: the same numbers
    step = min_nonzero(x) * min_nonzero(w)
    operands = [x / x_mul, w]
    tsum, tgrid = conv_terms(x, weff, G)
    if wino23:
        tsum, tgrid, planes = wino23_terms(x, weff, G)
        operands += planes
    grid, units = precheck(ref, tsum, tgrid, operands, step)
    return dict(x=x, w=w, ref=ref, grid=grid, units=units, step=step, weff=weff)


def wgrad_case(K, G, Cig, Cog, T, B, seed=0, insc=False, gy_mul=1.0):
    """gw of y = conv1d(x * in_scale, w): x [B, G*Cig, T], gy [B, G*Cog, T], in_scale [B, G*Cig] (or None)."""
    x, gy = lat((B, G * Cig, T), X_VALS, seed + 3), lat((B, G * Cog, T), X_VALS, seed + 4) * gy_mul
    sc = lat((B, G * Cig), R_VALS, seed + 5) if insc else None
    xin = x * sc[:, :, None] if insc else x
    ref = conv_bwd_weight(xin, gy, G, K)
    step = min_nonzero(xin) * min_nonzero(gy)
    tsum, tgrid = wgrad_terms(xin, gy, G, K)
    grid, units = precheck(ref, tsum, tgrid, [xin, gy / gy_mul], step)
    return dict(x=x, gy=gy, sc=sc, xin=xin, ref=ref, grid=grid, units=units, step=step)


def prologue_case(mode, G, Cig, Cog, T_out, P=3, Bp=2, seed=0, wino23=False):
    """Forward and weight gradient of y = conv1d(prologue(x), w) + bias, three passes with their own affine."""
    N = P * Bp
    Tin = T_out // 2 if mode & 2 else T_out
    x = lat((N, G * Cig, Tin), X_VALS, seed + 6)
    a, b = lat((P, G * Cig), PA_VALS, seed + 7), lat((P, G * Cig), PB_VALS, seed + 8)
    w, bias = lat((G * Cog, Cig, 3), W_VALS, seed + 9), lat((G * Cog,), R_VALS, seed + 10)
    gy = lat((N, G * Cog, T_out), X_VALS, seed + 11)
    xin = prologue(x, mode, a, b, Bp)
    ref = conv(xin, w, G, bias)
    step = min_nonzero(xin) * min_nonzero(w)
    tsum, tgrid = conv_terms(xin, w, G)
    operands = [x, a, b, w, bias, xin]
    if wino23:
        tsum, tgrid, planes = wino23_terms(xin, w, G)
        operands += planes
    grid, units = precheck(ref, tsum + float(bias.abs().max()), min(tgrid, grid_of(bias)), operands, step)
    gw = conv_bwd_weight(xin, gy, G, 3)
    wsum, wgrid_ = wgrad_terms(xin, gy, G, 3)
    gw_step = min_nonzero(xin) * min_nonzero(gy)
    gw_grid, gw_units = precheck(gw, wsum, wgrid_, [gy], gw_step)
    return dict(x=x, a=a, b=b, w=w, bias=bias, gy=gy, xin=xin, ref=ref, grid=grid, units=units, step=step,
                gw=gw, gw_grid=gw_grid, gw_units=gw_units, gw_step=gw_step)


def epilogue_case(T, which, B=2, V=3, K=3, seed=0, wino23=False):
    """test_conv_epilogue_and_views' chain on the lattice: one half (`which`) of every lead of enc [B, 128 V, T] through a strided
    view, in_scale, bias, residual, ReLU, a replayed mask with scale 1.25, a gate with scale 1.25; the weight gradient through the same
    view + in_scale; the backward-data launch, whose output goes into one half of a full tensor."""
    enc = lat((B, 128 * V, T), X_VALS, seed + 12)
    w = lat((128 * V, 64, K), W_VALS, seed + 13)
    bias, res = lat((128 * V,), R_VALS, seed + 14), lat((B, 128 * V, T), R_VALS, seed + 15)
    gate = lat((B, 128 * V, T), X_VALS, seed + 16)
    mask = keep_mask((B, 128 * V, T), seed + 17)
    scale = lat((B, 128 * V), R_VALS, seed + 18)
    gy = lat((B, 128 * V, T), X_VALS, seed + 19)
    xin = enc.view(B, V, 2, 64, T)[:, :, which].reshape(B, 64 * V, T)
    sc = scale.view(B, V, 2, 64)[:, :, which].reshape(B, 64 * V)
    xs = xin * sc[:, :, None]
    pre = conv(xs, w, V, bias)
    ref, _ = epilogue(pre, res=res, relu=True, mask=mask, drop_scale=DROP_SCALE, gate=gate, gate_scale=GATE_SCALE)
    step = min_nonzero(xs) * min_nonzero(w)
    tsum, tgrid = conv_terms(xs, w, V)
    operands = [enc, w, bias, res, scale, xs]
    if wino23:
        tsum, tgrid, planes = wino23_terms(xs, w, V)
        operands += planes
    # the epilogue's own terms: bias and residual enter the sum, the two scales of 1.25 = 5 / 4 refine the grid by 16
    tsum = (tsum + float(bias.abs().max()) + float(res.abs().max())) * DROP_SCALE * GATE_SCALE
    tgrid = min(tgrid, grid_of(bias), grid_of(res)) / 16
    grid, units = precheck(ref, tsum, tgrid, operands, step)
    assert float((ref == 0).double().mean()) > 0.2 and float((ref != 0).double().mean()) > 0.1      # every branch of the chain is taken
    gw = conv_bwd_weight(xs, gy, V, K)
    wsum, wgrid_ = wgrad_terms(xs, gy, V, K)
    gw_step = min_nonzero(xs) * min_nonzero(gy)
    gw_grid, gw_units = precheck(gw, wsum, wgrid_, [gy], gw_step)
    gx = conv_bwd_data(gy, w, V)
    gsum, ggrid_ = conv_terms(gy, launch_weight(w, V, True), V)
    gx_step = min_nonzero(gy) * min_nonzero(w)
    gx_grid, gx_units = precheck(gx, gsum, ggrid_, [gy], gx_step)
    return dict(enc=enc, w=w, bias=bias, res=res, gate=gate, mask=mask, scale=scale, gy=gy, ref=ref, grid=grid, units=units, step=step,
                gw=gw, gw_grid=gw_grid, gw_step=gw_step, gx=gx, gx_grid=gx_grid, gx_step=gx_step, xs=xs)


def scaled_block_case(B, G, C, T, seed=0):
    """test_conv_h2_channel_scaled_block_input's second half on the lattice: y = relu(conv(h, w2) + x * e) (res_scale), and the gated
    backward-data launch with a row scale and the per-(sample, channel) sums of (ungated gradient) x (gate) (stats_mode 1)."""
    x, h = lat((B, G * C, T), X_VALS, seed + 20), lat((B, G * C, T), X_VALS, seed + 21)
    e = lat((B, G * C), R_VALS, seed + 22)
    w = lat((G * C, C, 3), W_VALS, seed + 23)
    y, _ = epilogue(conv(h, w, G), res=x, res_scale=e, relu=True)
    tsum, tgrid = conv_terms(h, w, G)
    step = min_nonzero(h) * min_nonzero(w)
    grid, units = precheck(y, tsum + 4.0, tgrid, [x, h, e, w], step)
    gc, g2 = lat((B, G * C, T), X_VALS, seed + 24), lat((B, G * C, T), R_VALS, seed + 25)
    xr = F.relu(x)
    gated, pre = epilogue(conv_bwd_data(gc, w, G), res=g2, gate=xr, gate_scale=1.0, gate_rowscale=e)
    rows = (pre * xr).sum(2)                                               # [B, G*C]
    bsum, bgrid_ = conv_terms(gc, launch_weight(w, G, True), G)
    bsum = (bsum + 2.0) * 2.0
    g_grid, g_units = precheck(gated, bsum, bgrid_ / 2, [gc, g2, xr], step)
    r_grid, r_units = precheck(rows, float((pre.abs() * xr).sum(2).max()), grid_of(pre) * grid_of(xr), [], None)
    return dict(x=x, h=h, e=e, w=w, y=y, grid=grid, step=step, gc=gc, g2=g2, xr=xr, gated=gated, g_grid=g_grid, rows=rows, r_grid=r_grid)


def slot_case(G, Cin, Cout, T, B, flip=False, seed=0, P=1):
    """A launch whose epilogue leaves slot sums: (sum y, sum y^2) of its outputs, or -- a backward-data launch -- the
    BatchNorm-backward sums of the layer below, with dyadic statistics (mean in {-1, 0, 1}, invstd and a in {0.5, 1, 2}, b in
    {-1, 0, 1}: xhat = (x - mean) invstd is then on the lattice as well, so BOTH sums are exact)."""
    L = conv_launch(3, G, Cin, Cout, T, B, flip=flip, seed=seed)
    y = L["ref"]
    s = slot_sums(y)
    precheck(s[..., 0], float(slot_sums(y.abs())[..., 0].max()), L["grid"], [], None)
    precheck(s[..., 1], float(s[..., 1].max()), L["grid"] ** 2, [], None)
    L["slots"] = s
    if flip:
        Bp = B // P
        xb = lat((B, G * Cout, T), X_VALS, seed + 26)
        mean, invstd = lat((P, G * Cout), PB_VALS, seed + 27), lat((P, G * Cout), PA_VALS, seed + 28)
        a, b = lat((P, G * Cout), PA_VALS, seed + 29), lat((P, G * Cout), PB_VALS, seed + 30)
        bs = bn_backward_sums(y, xb, mean, invstd, a, b, Bp)
        ab = bn_backward_sums(y.abs(), xb, mean, invstd, a, b, Bp)
        e = lambda t: t.repeat_interleave(Bp, 0)[:, :, None]
        xh = (xb - e(mean)) * e(invstd)
        ab1 = slot_sums((y * xh).abs())[..., 0]
        precheck(bs[..., 0], float(ab[..., 0].max()), L["grid"], [xb, mean, invstd, a, b], None)
        precheck(bs[..., 1], float(ab1.max()), L["grid"] * grid_of(xh), [xh], None)
        L.update(xb=xb, mean=mean, invstd=invstd, a=a, b=b, Bp=Bp, bnb=bs)
    return L


def poly_case(G, Cig, Cog, T, B, aff, seed=0, P=1):
    """y = conv1d(upsample2(prologue(x)), w) + bias with x [B, G*Cig, T/2], and its two gradients.  The operands as the polyphase
    kernels multiply them: the half-resolution prologue output and the PHASE weights (0.25 / 0.75 combinations of the taps)."""
    Th = T // 2
    Bp = B // P
    x = lat((B, G * Cig, Th), X_VALS, seed + 31)
    w, bias = lat((G * Cog, Cig, 3), W_VALS, seed + 32), lat((G * Cog,), R_VALS, seed + 33)
    a, b = lat((P, G * Cig), PA_VALS, seed + 34), lat((P, G * Cig), PB_VALS, seed + 35)
    gy = lat((B, G * Cog, T), X_VALS, seed + 36)
    xp = prologue(x, 1, a, b, Bp) if aff else x
    u = upsample2(xp)
    ref = conv(u, w, G, bias)
    w0, w1, w2 = w[..., 0], w[..., 1], w[..., 2]
    phase = torch.stack([0.75 * w0 + 0.25 * w1, 0.25 * w0 + 0.75 * (w1 + w2), 0.25 * w2,
                         0.25 * w0, 0.25 * w2 + 0.75 * (w0 + w1), 0.75 * w2 + 0.25 * w1], 2)
    step = min_nonzero(u) * min_nonzero(w)
    tsum, tgrid = conv_terms(u, w, G)
    grid, units = precheck(ref, tsum + 2.0, min(tgrid, grid_of(xp) * grid_of(phase)), [x, w, bias, a, b, xp, phase, u], step)
    gx = upsample2_bwd(conv_bwd_data(gy, w, G))                            # wrt the prologue's output xp
    gsum, ggrid_ = conv_terms(gy, launch_weight(w, G, True), G)
    gx_step = 0.25 * min_nonzero(gy) * min_nonzero(w)
    gx_grid, _ = precheck(gx, 2.0 * gsum, ggrid_ / 4, [gy], gx_step)
    gw = conv_bwd_weight(u, gy, G, 3)
    wsum, wgrid_ = wgrad_terms(u, gy, G, 3)
    gw_step = min_nonzero(u) * min_nonzero(gy)
    gw_grid, _ = precheck(gw, wsum, wgrid_, [], gw_step)
    return dict(x=x, w=w, bias=bias, a=a, b=b, gy=gy, xp=xp, ref=ref, grid=grid, step=step, gx=gx, gx_grid=gx_grid, gx_step=gx_step,
                gw=gw, gw_grid=gw_grid, gw_step=gw_step, Bp=Bp)


def phase_major(gy):
    """gy [B, C, T] -> [B, 2C, T/2]: row 2c + p holds the outputs 2m + p of channel c (what bn_relu_bwd(phase_major=True) writes)."""
    B, C, T = gy.shape
    return gy.view(B, C, T // 2, 2).permute(0, 1, 3, 2).reshape(B, 2 * C, T // 2).contiguous()


def stem_case(B, V, L, seed=0):
    x, w = lat((B, V, L), X_VALS, seed + 37), lat((128 * V, 1, 15), W_VALS, seed + 38)
    ref = stem(x, w)
    gy = lat(tuple(ref.shape), X_VALS, seed + 39)
    gw = stem_bwd_weight(x, w, gy)
    precheck(ref, 15 * 2.0, 0.5, [x, w], 0.5)
    precheck(gw, float(gy.abs().sum((0, 2)).max()) * 2.0, 1.0, [gy], 1.0)
    return dict(x=x, w=w, ref=ref, gy=gy, gw=gw, grid=grid_of(ref), gw_grid=grid_of(gw), step=0.5, gw_step=1.0)


def convt2_case(B, G, T, seed=0):
    x, w, bias = lat((B, G * 128, T), X_VALS, seed + 40), lat((G * 128, 64, 2), W_VALS, seed + 41), lat((G * 64,), R_VALS, seed + 42)
    ref = convt2(x, w, bias, G)
    gy = lat(tuple(ref.shape), X_VALS, seed + 43)
    gx, gw, gb = convt2_grads(x, w, bias, gy, G)
    precheck(ref, 128 * 2.0 + 2.0, 0.5, [x, w, bias], 0.5)
    precheck(gx, 2 * 64 * 2.0, 0.5, [gy], 0.5)
    precheck(gw, B * T * 4.0, 1.0, [], 1.0)
    precheck(gb, B * 2 * T * 2.0, 1.0, [], 1.0)
    return dict(x=x, w=w, bias=bias, gy=gy, ref=ref, gx=gx, gw=gw, gb=gb)


# ------------------------------------------------------------------------------------------------ the case tables
# Tile extents, each from its kernel's own constant (csrc/conv_mfma.hip NT, WT; csrc/conv_h2.hip NTO; csrc/conv_h2w.hip TT;
# csrc/conv_bww_glds.hip TW).
NT, NTO, WT, TW, TT = 128, 256, 64, 32, 64
# forms of a forward / backward-data launch = nef_conv_args.wino of its packed operand
DIRECT, F23, F43, H2 = 0, 1, 2, 3
TILE = {DIRECT: NT, F23: NT, F43: NT, H2: NTO}


def _direct_cases():
    """(K, G, Cin, Cout, T, B, algo): `algo` "off" = split-fp16 and Winograd switched off, "on" = both on and the shape rules alone
    send the launch to the direct kernel (T = 66: even but under every other form's shortest row; T = 125: odd).  T below the 128-column
    tile packs several samples into one tile (segments of 16 .. 128 columns), so B = 5 puts sample seams inside it."""
    out = []
    for K in (1, 3, 7):
        for T in (1, 2, 7, 126, 127, 128, 129, 130, 258):
            out.append((K, 2, 64, 128, T, 5 if T < NT else 3, "off"))
        for T in (66, 125):
            out.append((K, 2, 64, 128, T, 5, "on"))
    # the 128-row tile of the direct kernel needs >= 384 column tiles x groups: 28 groups x 5 samples x 3 tiles
    out.append((3, 28, 64, 128, 258, 5, "off"))
    return out


DIRECT_CASES = _direct_cases()


def direct_wide(G, Cout, T, B):
    """nef_conv_fwd's rule for the 128-row tile of the direct (and F(2,3) / F(4,3)-less) kernel."""
    tiles = B * ((T + NT - 1) // NT) if T >= NT else -(-B // (NT // max(16, 1 << (T - 1).bit_length())))
    return Cout % 128 == 0 and G * (Cout // 128) * tiles >= 384


def _wino_cases():
    """(K, G, Cin, Cout, T, B, flip) for F(2,3) and F(4,3): 128 output channels per group from T = 128, 64 from T = 256; every T a
    single tile, a tile + 2, two tiles - 2, two tiles, two tiles + 2 of the 128-column tile."""
    out = []
    for K in (3, 7):
        for flip in (False, True):
            for T in (128, 130, 254, 256, 258):
                out.append((K, 2, 64, 128, T, 3, flip))
            for T in (256, 258):
                out.append((K, 2, 128, 64, T, 3, flip))
    return out


WINO_CASES = _wino_cases()
ZERO_TAIL = 40
ZERO_TAIL_CASES = [(3, 2, 128, 128, 256, 3), (7, 2, 128, 128, 256, 3)]      # K, G, Cin, Cout, T, B

H2_CASES = [(K, 2, 64, Cout, T, 2) for K in (1, 3, 7) for T in (128, 130, 254, 256, 258, 514) for Cout in (64, 128)]
PACKED_CASES = [(K, 2, 64, 128, T) for K in (1, 3) for T in (8, 12, 16, 32, 60, 64)]


def packed_batches(T):
    spt = (NTO + 4) // (T + 4)
    return spt, (1, spt, spt + 1, 2 * spt + 1)


PROLOGUE_CASES = [(mode, 2, 64, 128, T) for mode in (1, 2, 3) for T in (128, 130, 256, 258)]      # mode, G, Cig, Cog, T_out
EPILOGUE_CASES = [(T, which) for T in (130, 258) for which in (0, 1)]
SCALED_BLOCK_CASES = [(3, 2, 128, 130), (2, 1, 64, 258)]                                           # B, G, C, T
SLOT_CASES = [(2, 64, 128, 258, 3), (1, 128, 64, 514, 3), (2, 64, 64, 130, 3)]                     # G, Cin, Cout, T, B
WGRAD_CASES = [(K, 2, 64, Cog, T) for K in (3, 7) for T in (64, 66, 98, 126, 128, 130, 194) for Cog in (64, 128)]
WGRAD_BATCHES = (1, 2, 5)
WGRAD_DMA_CASES = [(3, 64, 1, 1, 64), (3, 66, 1, 1, 64), (3, 98, 2, 1, 64), (7, 64, 1, 1, 64), (7, 66, 1, 1, 64),
                   (7, 70, 2, 1, 64), (7, 130, 1, 2, 64)]                                          # K, T, B, G, C (T <= 516)


def wgrad_dma(K, Cig, Cog, T, mode=0, insc=False, passes=1):
    """nef_bww_glds_ok's rule: which form-4 weight gradients run on the LDS-DMA kernel."""
    return (not insc and (K == 3 or (K == 7 and not mode)) and not (mode & 2 and T % 4) and Cig % 64 == 0 and Cog % 64 == 0 and
            T >= 2 * TW and T % 2 == 0 and not (mode & 1 and passes > 8))


POLY_CASES = [(2, 64, 64, T, 3, aff) for T in (256, 258, 260, 514, 516) for aff in (False, True)]  # G, Cig, Cog, T, B, aff
STEM_SHAPES = [(2, 3, 500), (2, 1, 252), (2, 1, 244), (2, 2, 508), (70, 1, 12), (3, 2, 4), (2, 1, 8), (258, 1, 8)]
CONVT2_CASES = [(B, 2, 16) for B in (1, 5, 33)]                                                    # B, G, T
UPSAMPLE_TIN = (1, 2, 4, 65, 516)
MIX_V = (1, 2, 4, 8)
