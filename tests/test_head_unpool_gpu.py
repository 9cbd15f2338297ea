"""The mixes that un-pool inside the kernel (ops.lead_mean_mix_unpool / ops.mix_bwd_shared_unpool) against the op pairs they
replace -- roi_unpool_fwd + lead_mean_mix_shared and mix_bwd_shared_up + roi_unpool_bwd -- bit for bit, and against the CPU oracle."""
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


def _inputs(B, V, T, seed):
    z1, z2b = g(rnd(B, 128 * V, T, seed=seed)), g(rnd(B, 128 * V, 7, 32, seed=seed + 1))
    q, gD = g(rnd(B, 256, seed=seed + 2)), g(rnd(2 * B, 256, T, seed=seed + 3))
    return z1, z2b, q, gD


def _old_pair(o, z1, z2b, rois, q, gD, V, choice, T, relu, status=None):
    z2r = o.roi_unpool_fwd(z2b, rois, T, status)
    latent, D2 = o.lead_mean_mix_shared(z1, z2r, q, V, choice)
    gz1, gz2r, gq = o.mix_bwd_shared_up(gD, latent, z1, z2r, q, V, choice, relu_z1=relu)
    return latent, D2, gz1, o.roi_unpool_bwd(gz2r, rois), gq, z2r


def _gq_fp64(gD, latent, z1, z2r, V, choice):
    """gq[b, c] = sum_t ga*lat + gb*pick in fp64 from the fp32 inputs the kernels read."""
    B, T = latent.shape[0], latent.shape[2]
    c1, c2 = choice
    pick = torch.cat([z1[:, 128 * c1:128 * (c1 + 1)], z2r[:, 128 * c2:128 * (c2 + 1)]], 1).double()
    ga, gb = gD[:B].double(), gD[B:].double()
    return (ga * latent.double() + gb * pick).sum(2)


def _check(o, rois, B, V, T, choices, seed, tag):
    z1, z2b, q, gD = _inputs(B, V, T, seed)
    rois = g(rois)
    for choice in choices:
        cdev = torch.tensor(choice, dtype=torch.int32, device=DEV)
        for relu in (False, True):
            st_old = torch.zeros(1, dtype=torch.int32, device=DEV)
            latent, D2, gz1, gz2b, gq, z2r = _old_pair(o, z1, z2b, rois, q, gD, V, choice, T, relu, st_old)
            ref64 = _gq_fp64(gD, latent, z1, z2r, V, choice)
            for ch in (choice, cdev):
                st = torch.zeros(1, dtype=torch.int32, device=DEV)
                lat_f, D2_f = o.lead_mean_mix_unpool(z1, z2b, rois, q, V, ch, T, st)
                what = (tag, V, T, choice, relu, torch.is_tensor(ch))
                assert int(st.item()) == int(st_old.item()), what
                assert torch.equal(lat_f, latent), what
                assert torch.equal(D2_f, D2), what
                gz1_f, gz2b_f, gq_f = o.mix_bwd_shared_unpool(gD, lat_f, z1, z2b, rois, q, V, ch, relu_z1=relu)
                assert torch.equal(gz1_f, gz1), what
                assert torch.equal(gz2b_f, gz2b), what
                # gq: no further from fp64 than twice the two-pass form's own error (the bar for a different lane order) ...
                for rows in (slice(0, 256), slice(128, 256)):
                    e_old, e_new = rel(gq[:, rows], ref64[:, rows]), rel(gq_f[:, rows], ref64[:, rows])
                    print(f"gq {what} rows {rows.start}:{rows.stop} old {e_old:.3e} fused {e_new:.3e}")
                    assert e_new <= 2 * e_old, (what, e_old, e_new)
                # ... and in fact the same bits: the z1 half runs the same kernel, the z2 half deals positions to lanes as it does
                assert torch.equal(gq_f, gq), what


def _choices(V):
    return [c for c in ((0, 0), (V - 1, 0), (1, 2)) if max(c) < V]


@pytest.mark.parametrize("T", [64, 70, 1250, 65, 125, 7, 5, 4, 2])
@pytest.mark.parametrize("V", [1, 3, 12])
def test_unpool_mixes_equal_the_op_pairs(V, T):
    """T = 64: T % 4 == 0 (8-byte kernels); 70: T % 4 == 2 (the pair kernels); 1250: more than one 64-lane trip per segment;
    65, 125: odd (the scalar kernels, one position per lane; 125 is the latent row of a 500-sample beat); 7, 5, 4, 2: rows shorter
    than 8 deal their positions to the lanes one by one whatever their parity, and some of the seven segments are empty."""
    from electrocardio_panorama_amd import synth
    B = 3
    rois = torch.from_numpy(synth.make_rois(np.random.default_rng(5), B, 4 * T))
    _check(ops(), rois, B, V, T, _choices(V), 100 + V, "synth")


def test_unpool_mixes_when_a_wave_takes_several_rows():
    """More than twice as many (sample, channel) rows as the grid has waves (4096 blocks of 4): a wave then walks three rows,
    reuses its LDS strips and crosses from one sample's segment table to the next (128 rows per sample, 3 per wave)."""
    from electrocardio_panorama_amd import synth
    B, V, T = 258, 3, 70
    assert B * 128 > 2 * 4096 * 4
    rois = torch.from_numpy(synth.make_rois(np.random.default_rng(7), B, 4 * T))
    _check(ops(), rois, B, V, T, [(1, 2)], 150, "rows")


def test_unpool_mixes_on_the_golden_roi_cases(golden_dir):
    """Every recorded ROI table (empty segments, segments of 624 positions, T = 1250 with T % 4 == 2 among them)."""
    z = np.load(f"{golden_dir}/roi_cases.npz")
    names = sorted({k.split(":")[0] for k in z.files})
    assert names
    for name in names:
        rois = torch.from_numpy(z[f"{name}:rois"])
        _check(ops(), rois, rois.shape[0], 3, int(z[f"{name}:L"]) // 4, [(1, 2)], 200, name)


def test_unpool_mixes_on_a_malformed_roi_table():
    """Segments that run backwards and stop short of T: status is raised, everything else as the op pair leaves it."""
    o = ops()
    bad = torch.tensor([[[0, 100], [100, 90], [90, 200], [200, 300], [300, 400], [400, 450], [450, 500]]])
    B, V, T = 1, 3, 128
    z1, z2b, q, gD = _inputs(B, V, T, 300)
    st_old, st = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    latent, D2, gz1, gz2b, gq, _ = _old_pair(o, z1, z2b, g(bad), q, gD, V, (1, 2), T, True, st_old)
    lat_f, D2_f = o.lead_mean_mix_unpool(z1, z2b, g(bad), q, V, (1, 2), T, st)
    assert int(st_old.item()) == 1 and int(st.item()) == 1
    assert torch.equal(lat_f, latent) and torch.equal(D2_f, D2)
    gz1_f, gz2b_f, gq_f = o.mix_bwd_shared_unpool(gD, lat_f, z1, z2b, g(bad), q, V, (1, 2), relu_z1=True)
    assert torch.equal(gz1_f, gz1) and torch.equal(gz2b_f, gz2b)
    assert torch.equal(gq_f, gq)


def _off8(t):
    """The same values 8 bytes off a 16-byte boundary (test_shared_first_conv_pieces)."""
    buf = torch.empty(t.numel() + 2, device=DEV)
    v = buf[2:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


@pytest.mark.parametrize("T", [66, 1250])
def test_unpool_mixes_off_a_16_byte_boundary(T):
    """T % 4 == 2 on operands that are only 8-byte aligned: the un-pooling mixes fall back from the row-pair kernels to the 8-byte forms
    (and deal the z2 half's positions in pairs, not fours).  Same latent / D2 / gz1 / gz2b bits as the aligned run; gq, whose lane order
    follows the form, has the bits of the two-pass pair on the same misaligned operands.  (The outputs are the ops' own allocations:
    gz1 is 16-byte aligned in both runs, one misaligned operand is enough to leave the pair kernels.)"""
    from electrocardio_panorama_amd import synth
    o = ops()
    B, V, choice = 3, 3, (1, 2)
    rois = g(torch.from_numpy(synth.make_rois(np.random.default_rng(8), B, 4 * T)))
    z1, z2b, q, gD = _inputs(B, V, T, 400)
    z1o, gDo = _off8(z1), _off8(gD)
    lat, D2 = o.lead_mean_mix_unpool(z1, z2b, rois, q, V, choice, T)
    lat_o, D2_o = o.lead_mean_mix_unpool(z1o, z2b, rois, q, V, choice, T)
    assert torch.equal(lat_o, lat) and torch.equal(D2_o, D2)
    z2r = o.roi_unpool_fwd(z2b, rois, T)
    for relu in (False, True):
        gz1, gz2b, gq = o.mix_bwd_shared_unpool(gD, lat, z1, z2b, rois, q, V, choice, relu_z1=relu)
        gz1_o, gz2b_o, gq_o = o.mix_bwd_shared_unpool(gDo, _off8(lat), z1o, z2b, rois, q, V, choice, relu_z1=relu)
        assert torch.equal(gz1_o, gz1) and torch.equal(gz2b_o, gz2b), relu
        pair = o.mix_bwd_shared_up(gDo, _off8(lat), z1o, _off8(z2r), q, V, choice, relu_z1=relu)
        assert torch.equal(pair[0], gz1) and torch.equal(o.roi_unpool_bwd(pair[1], rois), gz2b), relu
        assert torch.equal(gq_o, pair[2]), relu
        assert rel(gq_o, gq) < 1e-6, relu


@pytest.mark.parametrize("L", [512, 500, 260, 28, 20, 8])
def test_unpool_mixes_against_the_oracle(L):
    """Against the CPU oracle's roi_unpool / lead_mean and autograd in fp64, at the bars test_mix and test_roi_backward_and_status
    hold the two-pass ops to (1e-6 forward, 1e-5 gradients).  T = 128; 125 and 65 (odd); 7, 5 and 2 (shorter than 8)."""
    o = ops()
    from oracle import nefnet_oracle as orc
    from electrocardio_panorama_amd import synth
    B, V, c1, c2 = 3, 3, 2, 1
    T = L // 4
    rois = torch.from_numpy(synth.make_rois(np.random.default_rng(6), B, L))
    z1f, zsf, qf = rnd(B, 128 * V, T, seed=50), rnd(B, 128 * V, 7, 32, seed=51), rnd(B, 256, seed=52)
    z1, zs, q = (t.double().requires_grad_(True) for t in (z1f, zsf, qf))
    z2r = orc.roi_unpool(zs, rois)
    assert z2r.dtype == torch.float64 and z2r.shape == (B, 128 * V, T)
    latent = torch.cat([orc.lead_mean(z1, V), orc.lead_mean(z2r, V)], 1)
    D2 = torch.cat([q[:, :, None] * latent,
                    q[:, :, None] * torch.cat([z1[:, 128 * c1:128 * (c1 + 1)], z2r[:, 128 * c2:128 * (c2 + 1)]], 1)], 0)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    lat_d, D2_d = o.lead_mean_mix_unpool(g(z1f), g(zsf), g(rois), g(qf), V, (c1, c2), T, st)
    assert int(st.item()) == 0
    assert rel(lat_d, latent) < 1e-6 and rel(D2_d, D2) < 1e-6
    gD = rnd(*D2.shape, seed=53)
    D2.backward(gD.double())
    gz1, gz2b, gq = o.mix_bwd_shared_unpool(g(gD), lat_d, g(z1f), g(zsf), g(rois), g(qf), V, (c1, c2))
    assert rel(gz1, z1.grad) < 1e-5 and rel(gz2b, zs.grad) < 1e-5 and rel(gq, q.grad) < 1e-5
