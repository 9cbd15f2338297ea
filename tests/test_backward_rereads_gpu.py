"""Two backward reductions formed by the kernel that already streams their tensor, against the entries they replace in the train step:
nef_bn_relu_bwd_outconv_w (the last conv's weight / bias gradient out of the last BatchNorm's sums pass) and nef_mix_bwd_unpool_rs
(chan_sum of gz1 out of the kernel that stores gz1).  Everything else those entries write must keep the parent entries' bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from util import rel, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from electrocardio_panorama_amd import ops as o
    return o


def g(t):
    return t.to(DEV).contiguous()


# ------------------------------------------------------------------ last conv's gradients from the BatchNorm sums pass
# (P, Bp, C, L).  (3, 2, 64, 8): one group pair per row, so both row-edge terms of the go window are exercised; (1, 5, 3, 1028): Bp not
# a multiple of the 8 splits, C < 64, a second trip of the 256-thread loop; (3, 9, 64, 2048): more rows than splits
OUTCONV_SHAPES = [(3, 2, 64, 8), (1, 5, 3, 1028), (3, 9, 64, 2048)]


def _outconv_case(P, Bp, Ct, L, seed=700):
    o = ops()
    N = P * Bp
    x = g(rnd(N, Ct, L, seed=seed))
    gamma, beta = g(rnd(Ct, seed=seed + 1) * 0.5 + 1.2), g(rnd(Ct, seed=seed + 2, scale=0.3))
    rm, rv = torch.zeros(Ct, device=DEV), torch.ones(Ct, device=DEV)
    mean, invstd, a, b = o.bn_train_stats(x, gamma, beta, rm, rv, P)
    w, bias = g(rnd(1, Ct, 3, seed=seed + 3, scale=0.2)), g(rnd(1, seed=seed + 4))
    out = o.outconv_fwd(x, w, bias, pro=(a, b, Bp))
    gout = g(rnd(N, 1, L, seed=seed + 5))
    neg = float((torch.addcmul(b.repeat_interleave(Bp, 0)[:, :, None], x, a.repeat_interleave(Bp, 0)[:, :, None]) <= 0).float().mean())
    assert 0.3 < neg < 0.7, neg      # about half of the ReLU decisions are negative
    return o, x, mean, invstd, a, b, w, out, gout


def _outconv_w_fp64(x, a, b, out, gout, P, Bp):
    """The definition (csrc/elementwise.hip, outconv_bwd_weight_partial's header) in fp64 from the fp32 tensors the kernels read:
    gw[c][k] = sum_{n,t} go[n][t] * x'[n][c][t+k-1], gb = sum go; go = gout*out*(1-out)/3, x' = max(0, x*a[p][c] + b[p][c])."""
    x, a, b, out, gout = (t.double().cpu() for t in (x, a, b, out, gout))
    go = gout * out * (1 - out) / 3                                        # [N, 1, L]
    xa = torch.clamp_min(x * a.repeat_interleave(Bp, 0)[:, :, None] + b.repeat_interleave(Bp, 0)[:, :, None], 0)
    xp = torch.nn.functional.pad(xa, (1, 1))
    L = x.shape[2]
    gw = torch.stack([(go * xp[:, :, k:k + L]).sum((0, 2)) for k in range(3)], 1)      # [C, 3]
    return torch.cat([gw.reshape(-1), go.sum().reshape(1)])


@pytest.mark.parametrize("P,Bp,Ct,L", OUTCONV_SHAPES)
def test_last_conv_gradients_from_the_bn_sums_pass(P, Bp, Ct, L):
    """gx, ggamma, gbeta, gx_chan_sum: the bits of nef_bn_relu_bwd form 1.  gw / gb: no further from fp64 than twice the error of
    nef_outconv_bwd_weight (affine prologue) on the same inputs -- the entry the train step called before; both errors are printed.
    Two calls give the same bits."""
    o, x, mean, invstd, a, b, w, out, gout = _outconv_case(P, Bp, Ct, L)
    ref = o.bn_relu_bwd_outconv(gout, out, w, x, mean, invstd, a, b, P)
    got = o.bn_relu_bwd_outconv(gout, out, w, x, mean, invstd, a, b, P, outconv_w=True)
    assert len(ref) == 4 and len(got) == 6
    for name, r, q in zip(("gx", "ggamma", "gbeta", "gx_chan_sum"), ref, got):
        assert torch.equal(r, q), name
    gw, gb = got[4], got[5]
    assert gw.shape == (1, Ct, 3) and gb.shape == (1,)
    gw_old, gb_old = o.outconv_bwd_weight(gout, out, x, pro=(a, b, Bp))
    ref64 = _outconv_w_fp64(x, a, b, out, gout, P, Bp)
    new, old = torch.cat([gw.reshape(-1), gb]), torch.cat([gw_old.reshape(-1), gb_old])
    e_new, e_old = rel(new, ref64), rel(old, ref64)
    print(f"outconv_w {(P, Bp, Ct, L)}: rel-L2 vs fp64  nef_outconv_bwd_weight {e_old:.3e}  from the sums pass {e_new:.3e}  "
          f"(gw alone {rel(gw_old, ref64[:-1]):.3e} / {rel(gw, ref64[:-1]):.3e}, gb alone {rel(gb_old, ref64[-1:]):.3e} / "
          f"{rel(gb, ref64[-1:]):.3e})")
    assert e_new <= 2 * e_old, (e_new, e_old)
    again = o.bn_relu_bwd_outconv(gout, out, w, x, mean, invstd, a, b, P, outconv_w=True)
    for r, q in zip(got, again):
        assert torch.equal(r, q)


def test_last_conv_gradients_entry_refuses_what_it_does_not_serve():
    """Wrong form: NEF_E_UNSUPPORTED (-4); NULL outputs or workspace: NEF_E_NULL (-2); a short second workspace: NEF_E_WORKSPACE (-3) --
    all before anything is launched."""
    from electrocardio_panorama_amd import _lib
    P, Bp, Ct, L = 1, 2, 3, 8
    o, x, mean, invstd, a, b, w, out, gout = _outconv_case(P, Bp, Ct, L)
    lib = _lib.load()
    p = o._p
    gx, gg, gbt = torch.empty_like(x), torch.empty(Ct, device=DEV), torch.empty(Ct, device=DEV)
    gw, gb = torch.full((1, Ct, 3), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)

    def args(**kw):
        A = _lib.BnBwdArgs(x=p(x), mean=p(mean), invstd=p(invstd), a=p(a), b=p(b), gx=p(gx), ggamma=p(gg), gbeta=p(gbt), P=P, Bp=Bp,
                           C=Ct, L=L, form=1, gout=p(gout), out=p(out), wout=p(w))
        for k, v in kw.items():
            setattr(A, k, v)
        A.ws_bytes = max(lib.nef_bn_bwd_ws_bytes(C.byref(A)), 1 << 16)
        A.ws = p(ws)
        return A

    ws, ws2 = torch.empty(1 << 16, dtype=torch.uint8, device=DEV), torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    n2 = lib.nef_bn_relu_bwd_outconv_w_ws_bytes(C.byref(args()))
    assert n2 == P * Ct * 8 * 4 * 8
    assert lib.nef_bn_relu_bwd_outconv_w_ws_bytes(C.byref(args(form=0))) == 0
    call = lib.nef_bn_relu_bwd_outconv_w
    for form in (0, 2, 3, 9):
        assert call(C.byref(args(form=form, gout=None, out=None, wout=None, g=p(gx))), p(gw), p(gb), p(ws2), n2, None) == -4, form
    assert call(None, p(gw), p(gb), p(ws2), n2, None) == -2
    assert call(C.byref(args()), None, p(gb), p(ws2), n2, None) == -2
    assert call(C.byref(args()), p(gw), None, p(ws2), n2, None) == -2
    assert call(C.byref(args()), p(gw), p(gb), None, n2, None) == -2
    assert call(C.byref(args()), p(gw), p(gb), p(ws2), n2 - 1, None) == -3
    torch.cuda.synchronize()
    assert float(gw.min()) == 7.0 and float(gb.min()) == 7.0      # nothing was launched
    assert call(C.byref(args()), p(gw), p(gb), p(ws2), n2, None) == 0
    torch.cuda.synchronize()
    assert float(gw.max()) != 7.0


# ------------------------------------------------------------------ chan_sum(gz1) from the kernel that stores gz1
# (B, V, T), T % 4 == 2: the pair kernel, a vector straddling two rows; T / 4 below and above 64.  T % 4 == 0: the fallback
MIX_SHAPES = [(2, 3, 10, True), (3, 2, 250, True), (2, 3, 1250, True), (2, 3, 64, False)]


def _mix_inputs(B, V, T, seed):
    from electrocardio_panorama_amd import synth
    z1 = g(torch.clamp_min(rnd(B, 128 * V, T, seed=seed), 0))      # a ReLU output: exact zeros in about half the places
    assert 0.3 < float((z1 == 0).float().mean()) < 0.7
    z2b, q, gD = g(rnd(B, 128 * V, 7, 32, seed=seed + 1)), g(rnd(B, 256, seed=seed + 2)), g(rnd(2 * B, 256, T, seed=seed + 3))
    rois = g(torch.from_numpy(synth.make_rois(np.random.default_rng(seed), B, 4 * T)))
    latent, _ = ops().lead_mean_mix_unpool(z1, z2b, rois, q, V, (1, 0), T)
    return z1, z2b, q, gD, rois, latent


@pytest.mark.parametrize("B,V,T,in_kernel", MIX_SHAPES)
def test_gz1_channel_sum_from_the_mix_backward(B, V, T, in_kernel):
    """gz1, gz2b, gq: the bits of nef_mix_bwd_unpool.  The channel sum: no further from the fp64 sum of the stored gz1 than twice the
    error of nef_chan_sum on it; both errors are printed.  Two calls give the same bits; the entry says which kernel formed the sum."""
    from electrocardio_panorama_amd import _lib
    o = ops()
    z1, z2b, q, gD, rois, latent = _mix_inputs(B, V, T, 800 + T)
    choice = (1, 0)
    ref = o.mix_bwd_shared_unpool(gD, latent, z1, z2b, rois, q, V, choice, relu_z1=True)
    got = o.mix_bwd_shared_unpool(gD, latent, z1, z2b, rois, q, V, choice, relu_z1=True, chan_sum=True)
    assert len(ref) == 3 and len(got) == 4
    for name, r, c in zip(("gz1", "gz2b", "gq"), ref, got):
        assert torch.equal(r, c), name
    gz1, cs = got[0], got[3]
    assert cs.shape == (128 * V,)
    assert float((gz1 == 0).float().mean()) > 0.3      # the relu_z1 mask is in what was summed
    ref64 = gz1.double().sum((0, 2)).cpu()
    e_new, e_old = rel(cs, ref64), rel(o.chan_sum(gz1), ref64)
    print(f"gz1 chan_sum {(B, V, T)}: rel-L2 vs fp64  nef_chan_sum {e_old:.3e}  from the mix backward {e_new:.3e}")
    assert e_new <= 2 * e_old, (e_new, e_old)
    again = o.mix_bwd_shared_unpool(gD, latent, z1, z2b, rois, q, V, choice, relu_z1=True, chan_sum=True)
    for r, c in zip(got, again):
        assert torch.equal(r, c)
    # the entry itself: which path it took, and a device-side choice gives the same result
    lib, p = _lib.load(), o._p
    outs = [torch.empty_like(t) for t in got]
    n = lib.nef_mix_bwd_unpool_rs_ws_bytes(B, V)
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=DEV)
    took = C.c_int(-1)
    cdev = torch.tensor(choice, dtype=torch.int32, device=DEV)
    rc = lib.nef_mix_bwd_unpool_rs(p(gD), p(latent), p(z1), p(z2b), p(rois), p(q), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(ws), n,
                                   C.byref(took), B, V, T, 0, 0, p(cdev), 1, None)
    assert rc == 0 and took.value == int(in_kernel)
    for r, c in zip(got, outs):
        assert torch.equal(r, c)
    assert lib.nef_mix_bwd_unpool_rs(p(gD), p(latent), p(z1), p(z2b), p(rois), p(q), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(ws),
                                     n - 1, None, B, V, T, 1, 0, None, 1, None) == -3
    assert lib.nef_mix_bwd_unpool_rs(p(gD), p(latent), p(z1), p(z2b), p(rois), p(q), p(outs[0]), p(outs[1]), p(outs[2]), None, p(ws),
                                     n, None, B, V, T, 1, 0, None, 1, None) == -2
