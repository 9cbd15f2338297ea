"""Tie-aware gradient parity (test helper).

A backward pass is discontinuous at every ReLU and L1 residual whose argument sits at the switching point.  Instead of
loosening the gradient bar for such ties, the oracle REPLAYS the discrete decisions the HIP path took
(`oracle.Decisions`), the test asserts that every decision the oracle itself would have taken differently is a genuine
tie (pre-activation at round-off level relative to that site's scale), and the gradients are then held to the
tie-free bars: flat <= 1e-4, per tensor <= 1e-3 rel-L2."""
import torch

from util import rel

FLAT_TOL, TENSOR_TOL = 1e-4, 1e-3
# A flipped decision must have |pre-activation| <= TIE_REL * rms(pre-activation of its site).  2e-5 = twice the largest
# ratio seen over every replaying test incl. the 5e9 decisions of the full-size step (profiles/r03_tie_ratios.md); the
# round-2 value was 1e-4.
TIE_REL = 2e-5
TIE_FRAC = 1e-5           # and flips must be rare: <= TIE_FRAC * numel + 2 per site
DEGENERATE_FRAC = 1e-4    # cap on the exact-zero flips that are exempt from TIE_FRAC on the F(4,3)-forward sites


def _pos(t):
    return (t > 0).cpu()


def gpu_decisions(model, outs, target, keep_masks=None, reg_l1=True, fold=None):
    """Decision masks of the last train-phase forward of `model` (needs model.keep_saved = True before the call).
    `fold=(B, V)`: Model_nefnet2 -- the encoder ran on the lead-folded batch (row n = v*B + b); its sites are emitted
    per lead as "<site>@<v>"."""
    sv = model.last_saved
    assert sv is not None, "set model.keep_saved = True before the forward"
    dm = {}

    def emit(site, full):
        """`full`: bool tensor over the (folded) batch, or callable(own rows, row slice) -> decision."""
        if fold is None:
            dm[site] = full if not callable(full) else (lambda own, f=full: f(own, slice(None)))
            return
        B, V = fold
        for v in range(V):
            rows = slice(v * B, (v + 1) * B)
            dm[f"{site}@{v}"] = full[rows] if not callable(full) else (lambda own, f=full, rows=rows: f(own, rows))

    def block(saved, window=None):
        h, y, prefix = saved[1], saved[2], saved[3]
        h1, y1 = _pos(h), _pos(y)
        keep = None if keep_masks is None else keep_masks[prefix].bool()
        if window is None:
            if keep is None:
                emit(prefix + ".relu1", h1)
            else:       # dropped positions (keep == 0) carry no decision: leave the oracle's own there
                emit(prefix + ".relu1", lambda own, rows: torch.where(keep[rows], h1[rows], own))
            emit(prefix + ".relu2", y1)
            return
        # the block ran on a 6-sample window: h is exact on window columns 1..4, y on columns 2..3 (the two rows
        # roi_algin reads); everything else keeps the oracle's own decision and carries no gradient
        t0 = window[0]

        def r1(own, rows):
            m = own.clone()
            sl = slice(t0 + 1, t0 + 5)
            hw_ = h1[rows][:, :, 1:5]
            m[:, :, sl] = hw_ if keep is None else torch.where(keep[rows][:, :, sl], hw_, own[:, :, sl])
            return m

        def r2(own, rows):
            m = own.clone()
            m[:, :, t0 + 2:t0 + 4] = y1[rows][:, :, 2:4]
            return m
        emit(prefix + ".relu1", r1)
        emit(prefix + ".relu2", r2)

    for s in sv["blk_enc"]:
        block(s)
    for key in ("blk_w_conv", "blk_z1", "blk_c20", "blk_c22"):
        block(sv[key])
    block(sv["blk_z2c"], sv["z2_win"])
    saved, passes = sv["dec"][0], sv["dec"][3]
    names = ("decoder.1.double_conv.1", "decoder.1.double_conv.4", "decoder.3.double_conv.1", "decoder.3.double_conv.4")
    for li, ent in enumerate(saved):
        c, a, b = ent[1], ent[4], ent[5]
        Bp = c.shape[0] // passes
        for p in range(passes):
            pre = torch.addcmul(b[p].double().view(1, -1, 1), c[p * Bp:(p + 1) * Bp].double(), a[p].double().view(1, -1, 1))
            dm[f"pass{p}.{names[li]}"] = _pos(pre)
    o, op, ol = (t.detach() for t in outs)
    dm["loss1"] = torch.sign(o - op).cpu()
    dm["loss2"] = torch.sign(o - ol).cpu()
    if reg_l1:
        dm["loss3"] = torch.sign(o - target.to(o.device)).cpu()
    return dm


TIE_LOG = []              # (site, worst / rms, flips, numel) of every site with a flip, for tools/tie_ratios.py


def assert_flips_are_ties(dec):
    """Replayed decisions that differ from the oracle's own must be ties: the oracle's argument within TIE_REL of the
    switching point (relative to the site's rms) and rare (<= TIE_FRAC * numel + 2 per site).  Flips where the oracle's
    argument is EXACTLY zero (the all-zero tail of a beat seen through a conv) are exempt from the rarity bound only on
    sites whose forward conv runs through F(4,3) -- the decoder passes -- and on the L1 sign sites: F(4,3) computes such
    an output from products that cancel only analytically.  Every encoder-side forward conv takes F(2,3) or the direct
    form, which keep the reference's exact 0.0 by construction (each product feeding an output only sees that output's
    receptive field): there an exact-zero flip is counted like any other flip.  (It cannot be required to be absent: one
    genuine tie upstream that the HIP path resolved as 1e-9 instead of 0 turns an exact 0 of the oracle one layer
    down into a +-1e-9 -- 1 such position among 1.2e8 in the full-size step.)"""
    for site, r in dec.report.items():
        if r["flips"] == 0:
            continue
        TIE_LOG.append((site, r["worst"] / max(r["rms"], 1e-30), r["flips"], r["numel"]))
        f4_forward = site.startswith("pass") or site.startswith("loss")
        assert r["flips"] - (r.get("degenerate", 0) if f4_forward else 0) <= TIE_FRAC * r["numel"] + 2, (site, r)
        # the exemption is not a blank cheque: exact-zero flips are bounded too (largest share seen: 705 of 512 k = 1.4e-3 in
        # one encoder block when F(4,3) was tried there; on the decoder sites of the shipped path <= 2e-5)
        assert r.get("degenerate", 0) <= DEGENERATE_FRAC * r["numel"] + 2, (site, r)
        assert r["worst"] <= TIE_REL * max(r["rms"], 1e-30), (site, r)


def assert_grad_parity(named_grads, P_ref, dead=(), zero_abs=None, flat_tol=FLAT_TOL, tensor_tol=TENSOR_TOL, n_terms=1e4, zero_floor=None):
    """named_grads: {name: HIP gradient}; P_ref: oracle params with .grad.  `zero_abs`: names whose gradient is
    analytically zero -- the conv biases in front of a train-mode BatchNorm: both sides only hold the
    rounding residue of a sum of ~N cancelling terms, so the HIP value is held to an ABSOLUTE bar that scales like that
    residue: 1e-6 * max(1, sqrt(n_terms / 1e4)) times the scale of the summed terms (the matching BatchNorm-bias gradient,
    a sum over the same N positions).  `zero_floor`: {name: absolute bar} that replaces a smaller one -- a measured residue of the
    same sum (tests/test_lengths_gpu.py: a BatchNorm over four values has an invstd, and so terms, far above its bias gradient)."""
    zero_abs = zero_abs or (lambda k: k.endswith("double_conv.0.bias") or k.endswith("double_conv.3.bias"))
    got, want, worst = [], [], (0.0, None)
    for k, v in P_ref.items():
        if k in dead:
            assert named_grads.get(k) is None, k
            continue
        g = named_grads[k].detach().double().cpu()
        r = v.grad.detach().double()
        if zero_abs(k):
            bn_bias = k[:-len("0.bias")] + ("1.bias" if k.endswith("double_conv.0.bias") else "4.bias")
            scale = max(1.0, float(P_ref[bn_bias].grad.detach().abs().max()))
            bar = max(1e-6 * max(1.0, (n_terms / 1e4) ** 0.5) * scale, (zero_floor or {}).get(k, 0.0))
            assert float(g.abs().max()) < bar and float(r.abs().max()) < 10 * bar, (k, float(g.abs().max()), float(r.abs().max()), bar)
            continue
        e = rel(g, r)
        if e > worst[0]:
            worst = (e, k)
        got.append(g.reshape(-1))
        want.append(r.reshape(-1))
    flat = rel(torch.cat(got), torch.cat(want))
    assert flat < flat_tol, (flat, worst)
    assert worst[0] < tensor_tol, worst
    return flat, worst
