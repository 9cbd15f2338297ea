/* nefnet_hip.h -- C ABI of libnefnet_hip.so: the gfx950 (MI355X) kernels of the Nef-Net train step.
 *
 * The reference (WhatAShot/Electrocardio-Panorama) has no FFI of its own: every op below replaces an
 * implicit PyTorch call site on the hot path, cited per entry as `codes/<file>:<line>`.  The Python
 * host (`electrocardio_panorama_amd/network`) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates;
 *   - activations are fp32 `[batch][channel][time]`, time contiguous; ROIs are int64 `[B][7][2]`;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises,
 *     every entry point is re-entrant and hipGraph-capturable; the only thing the library remembers is, per kernel and
 *     per device, that its dynamic-LDS limit has been raised (an idempotent, atomically published flag);
 *   - return 0 on success, a negative NEF_E_* for a rejected call, a positive value = hipError_t.
 */
#ifndef NEFNET_HIP_H
#define NEFNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NEF_OK 0
#define NEF_E_SHAPE (-1)        /* a dimension is out of the supported set */
#define NEF_E_NULL (-2)         /* a required pointer is NULL */
#define NEF_E_WORKSPACE (-3)    /* workspace too small */
#define NEF_E_UNSUPPORTED (-4)  /* configuration not built */

#define NEF_N_SEG 7    /* heartbeat segments per sample (codes/dataset/tianchi.py:103-106) */
#define NEF_ROI_BINS 16 /* roi_algin size (codes/network/model_nefnet.py:136) */

typedef void* nef_stream_t;

/* ABI version of this header; bumped on any signature change. */
int nef_abi_version(void);   /* 22 (+ nef_flatten_acc, nef_lr_sched / nef_lr_sched_args_bytes, nef_loss_ssim_fwd / nef_loss_ssim_bwd / nef_loss_ssim_ws_bytes / nef_loss_ssim_args_bytes, nef_loss_seg_fwd / nef_loss_seg_bwd / nef_loss_seg_ws_bytes / nef_loss_seg_args_bytes / nef_view_seg_metrics, nef_loss_slope_fwd / nef_loss_slope_bwd / nef_loss_slope_ws_bytes / nef_loss_slope_args_bytes / nef_view_slope_metrics, nef_loss_corr_fwd / nef_loss_corr_bwd / nef_loss_corr_ws_bytes / nef_loss_corr_args_bytes / nef_view_corr_metrics, nef_locate_score / nef_locate_best / nef_locate_cands and their _args_bytes, nef_beat_batch / nef_beat_batch_args_bytes: additions only, the number stays; a binding finds a library without them by the missing symbol.  Weight packing is ONE entry, nef_pack_weights(nef_pack_desc*, n), + nef_pack_bytes(nef_pack_desc*) for the size of any operand.  ABI <= 21 had nef_pack_weight, nef_pack_weight_wino, nef_pack_weight_wino4, nef_pack_weight_h2 and nef_pack_weight_h2_bytes: each is one descriptor with wino = 0 / 1 / 2 / 3); 21 (BatchNorm backward is ONE entry on a nef_bn_bwd_args struct, + nef_bn_bwd_args_bytes; nef_mix_bwd takes `up` / `shared` flags; nef_outconv_fwd / nef_outconv_bwd_weight take the prologue arguments.  ABI <= 20 had nef_bn_relu_bwd_phase_major, nef_bn_relu_bwd_up, nef_bn_relu_bwd_combine3, nef_bn_relu_bwd_combine3_phase_major, nef_bn_relu_bwd_outconv, nef_bn_bwd_outconv_ws_bytes, nef_mix_bwd_up, nef_mix_bwd_shared, nef_mix_bwd_shared_up, nef_outconv_fwd_pro and nef_outconv_bwd_weight_pro); 20 (the weight gradient is ONE entry, nef_conv_bwd_weight(nef_bww_args*), + nef_bww_args_bytes; its _pro, _wino4, _h2 and _h2_ws_bytes variants are gone); 19 (+ nef_adam, nef_h2_tail_census, nef_bwd_weight_clamp_ends: additions only; the kernel-form option entry points of 16 and nef_upsample2_aff_fwd are gone; + nef_debug_spin_us); 18 (round 6: nef_pack_desc + src_mode / src_Cr (polyphase weights synthesized inside the pack), + nef_amax_roll, nef_flatten, nef_regroup_halves, nef_step_words, nef_pano_h_conv_tail, + num_batches_tracked in the three BatchNorm statistics entry points, nef_pano_h_conv_pair for any length); 17 (round 5: + pro_mode 4 / 8 / 9, nef_poly_weights, nef_poly_fwd_edge, nef_poly_bwd_edge, nef_mix_bwd_shared: polyphase forward / backward-data through the x2 upsampling); 16 (round 5: + kernel-form option entry points); 15 (round 4: + x_clamped / clamped counters); 14 (round 4: + the split-fp16 weight gradient, now form 3); 13 (round 4: + nef_pack_weight_h2 / conv args wino = 3 and x_scale: direct convolutions on exact fp16 splits of the fp32 operands); 12 (round 4: nef_conv_bwd_weight_wino -- the transposed F(3,2) weight gradient -- is gone, the transposed F(3,4) / F(4,4) entry, now form 4, covers every shape it took; 11, round 3: the K = 7 F(4,.) operand has 13 planes, Winograd operands are laid out as 16-byte vectors; 10: + nef_pano_h_conv_pair) */

/* Diagnostics: `wgs` workgroups busy for `us` microseconds on `stream` (a stand-in for a collective's time on the chip:
 * parallel.DryCollective, bench.py --dry-collective).  0 <= us <= 50000, 1 <= wgs <= 64. */
int nef_debug_spin_us(float us, int wgs, nef_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Stem: Conv1d(1->128 per lead, k15, s2, p7, no bias) + ReLU + MaxPool1d(3,2,1), fused.
 * Replaces codes/network/encoder/encoder.py:35-38 (resnet_1d.py:102-105).
 *   x [B][V][L], w [128V][1][15], y [B][128V][L/4]; L % 4 == 0.
 * bwd_weight recomputes the conv, routes gy through the pool arg-max and the ReLU.
 *   ws: nef_stem_bwd_ws_bytes(V) bytes of scratch. */
int nef_stem_fwd(const float* x, const float* w, float* y, int B, int V, int L, nef_stream_t stream);
/* Live extent of the stem's output, measured on the tensor the stem reads: live[b*V + v] (int32) = the first pooled position from
 * which row (b, v) of nef_stem_fwd's output is exactly zero, in all 128 channels.  With e = 1 + index of the row's last element
 * x != 0.f (-0.f counts as zero, NaN as non-zero; an all-zero row: e = 0):
 *   cj = e ? min(L/2, (e+6)/2 + 1) : 0,   live = cj ? min(L/4, cj/2 + 1) : 0
 * (conv output j reads x[2j-7 .. 2j+7], pooled output t covers j = 2t-1 .. 2t+1; no bias, so ReLU(0) = 0 behind them).
 * A bias-free conv of kernel size K widens the extent by (K-1)/2 and no more: nef_conv_fwd_live takes the table + that addend.
 * One small launch, no host read; L % 4 == 0. */
int nef_live_extent(const float* x, int32_t* live, int B, int V, int L, nef_stream_t stream);
size_t nef_stem_bwd_ws_bytes(int V);
int nef_stem_bwd_weight(const float* x, const float* w, const float* gy, float* gw, void* ws, size_t ws_bytes,
                        int B, int V, int L, nef_stream_t stream);
/* The same with nef_live_extent's table of the same x (live [B][V], required): behind a row's extent the conv's pre-activations are
 * exactly zero, so the ReLU gate kills gy there whatever it holds; the matrix-core kernel (L % 8 == 0, row within 64 KiB of LDS) walks
 * and stages every row only up to its extent rounded up to 16 outputs.  Same bits; the other kernel ignores the table. */
int nef_stem_bwd_weight_live(const float* x, const float* w, const float* gy, float* gw, void* ws, size_t ws_bytes,
                             int B, int V, int L, const int32_t* live, nef_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Grouped Conv1d (stride 1, odd K in {1,3,7}, pad (K-1)/2) as an implicit GEMM on fp32 MFMA.
 * Replaces nn.Conv1d at codes/network/model_nefnet.py:18,21,32,44 and encoder/resnet_1d.py:23.
 *
 * nef_pack_weights packs the operands of nef_conv_fwd: any number in one call (a whole train step packs ~50), one
 * descriptor each; `descs` is a HOST array.  w [G*Cog][Cig][K] (torch layout) -> wp, nef_pack_bytes(desc) bytes, in the
 * form `wino` names -- the value the conv launch then passes as nef_conv_args.wino.  transpose_flip = 1 packs the
 * backward-data operand: (ci, co) exchanged and the taps reversed.
 *
 * wino = 0, the direct kernels: G*Cog*Cig*K floats.
 *   transpose_flip = 0: forward operand   wp[g][k][ci][co] = w[g*Cog+co][ci][k]
 *   transpose_flip = 1: bwd-data operand  wp[g][k][co][ci] = w[g*Cog+co][ci][K-1-k]
 *
 * wino = 1, Winograd F(2,3), K == 3 or 7.
 * K == 3: wp[g][plane][ci][co], 4 planes (g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2) of the taps w[g*Cog+co][ci][0..2].
 * K == 7 (taps split 4 + 3): 10 planes = the F(2,4) transform of taps 0..3 (g0/2, -(g0+g1+g2+g3)/2, (-g0+g1-g2+g3)/6,
 * (g0+2g1+4g2+8g3)/6, g3), the F(2,3) transform of taps 4..6 with its last plane negated, one plane of padding, laid out for
 * 16-byte fragment loads: wp[g][q][ci][co / 64][co % 32][4] with value 2*plane + (co % 64) / 32 = 4*q + e (conv_mfma.hip).
 * The layout is private to nef_conv_fwd; the size is planes * G * Cog * Cig floats either way.
 *
 * wino = 2, the F(4,3) operand, K == 3 or 7: 6 planes for K == 3 -- (g0/4, -(g0+g1+g2)/6, -(g0-g1+g2)/6, g0/24+g1/12+g2/6,
 * g0/24-g1/12+g2/6, g2) -- and 13 for K == 7: taps split 4 + 3, the F(4,4) transform of taps 0..3 (7 planes, points 0, +-1,
 * +-2, inf, 1/2) followed by the F(4,3) transform of taps 4..6.  Stored as slabs of 16-byte vectors,
 * wp[g][plane / 4][ci][co / 32][co % 32][4] plus a tail slab for the planes % 4 last planes (conv_mfma.hip); planes * G *
 * Cog * Cig floats.
 *
 * wino = 3, the split-fp16 operand: each weight, scaled by a power of two per output row of the launch (row
 * maximum -> [2^14, 2^15)), is split exactly into two fp16 terms w = wh + wl (+ < 2^-22 |w|) and stored as matrix-core
 * fragments wp[g][ci/16][k][co/32][wh | wl][lane][8] (fp16), followed by the per-row descale factors [g][co] (fp32):
 * G*K*Cog*Cig floats plus one word per output row of the launch.
 * nef_conv_fwd then runs the DIRECT convolution as three v_mfma_f32_32x32x16_f16 per 16 channels and tap -- xh*wh + xh*wl +
 * xl*wh, exact fp16 products, fp32 accumulation (csrc/conv_h2.hip): fp32-class results (1.1e-7 rel-L2 on a 128-channel K = 7
 * layer against fp64; an fp32 direct conv: 1.3e-7) at 3/16 of the fp32 matrix instructions' pipe time.  K == 1, 3 or 7, Cig % 16 == 0,
 * Cog % 32 == 0 (both as the LAUNCH sees them: exchanged under transpose_flip). */
typedef struct nef_pack_desc {
    const float* w;
    float* wp;
    int32_t G, Cog, Cig, K, transpose_flip, wino;
    /* round 6, wino = 3 only: how the packed tensor [G*Cog][Cig][K] is read out of `w`.  0: `w` is that tensor.  1: `w` is
     * [G*Cog/2][Cig][3] and the packed tensor holds the two PHASE weights of each row (conv1d(upsample2(x), w) as two K = 3 convs on the
     * half-resolution x, codes/network/model_nefnet.py:102-105 -- what nef_poly_weights would write, formed inside the pack so the
     * phase tensor is never materialised); src_Cr = 0: row 2 r + p, src_Cr = Cog/2 > 0: the tile order of the polyphase forward launch. */
    int32_t src_mode, src_Cr;
} nef_pack_desc;
/* Bytes of the operand `d` packs (w and wp are not looked at); 0 for a descriptor nef_pack_weights rejects by shape or form. */
size_t nef_pack_bytes(const nef_pack_desc* d);
int nef_pack_weights(const nef_pack_desc* descs, int n, nef_stream_t stream);

typedef struct nef_conv_args {
    const float* x;        /* input  [B][..][T]; element (b, g, ci, t) at x + b*x_bs + g*x_gs + ci*T + t */
    const float* wp;       /* packed weights (nef_pack_weights; wino 0: [G][K][Cin_g][Cout_g]) */
    float* y;              /* output; element (b, g, co, t) at y + b*y_bs + g*y_gs + co*T + t */
    const float* bias;     /* [G*Cout_g] or NULL */
    const float* in_scale; /* NULL, or per (sample, input channel) factor at in_scale + b*sc_bs + g*sc_gs + ci */
    const float* res;      /* NULL, or residual added before the activation, laid out like y with res_bs/res_gs */
    const float* gate;     /* NULL, or y *= gate_scale * (gate > 0), laid out like y with gate_bs/gate_gs */
    const uint8_t* mask;   /* NULL, or dropout keep-mask (0/1), dense [B][G*Cout_g][T]; y *= mask * drop_scale */
    int64_t x_bs, x_gs, y_bs, y_gs, sc_bs, sc_gs, res_bs, res_gs, gate_bs, gate_gs;
    int32_t B, T, G, Cin_g, Cout_g, K;
    int32_t relu;          /* apply max(0, .) after bias + residual */
    float gate_scale;
    float drop_scale;      /* 1/(1-p); with mask == NULL and drop_p > 0 the keep-mask comes from the counter RNG */
    float drop_p;
    uint64_t rng_seed;     /* counter RNG: keep(b, channel, t) = hash(seed, dense index) >= p */
    /* Input prologue, applied while the activation tile is staged (decoder fusion, K == 3 only):
     *   pro_mode bit0: x' = max(0, x*pro_a[p][ch] + pro_b[p][ch]) with p = sample / pro_Bp -- the BatchNorm affine + ReLU
     *                  of the producing layer (model_nefnet.py:19-23); pro_a/pro_b are [P][G*Cin_g];
     *   pro_mode bit1: the input is stored at half resolution [..][T/2] and is x2-upsampled on the fly exactly as
     *                  nn.Upsample(scale_factor=2, mode='linear', align_corners=False) (model_nefnet.py:102,104);
     *                  x_bs / x_gs and the channel pitch then refer to the half-resolution tensor.
     *   pro_mode 8 / 9 (wino == 3 only): polyphase forward of conv1d(upsample2(x)) -- x at half resolution [..][T], Cout_g = 2 x the
     *                  conv's channels (tile-ordered phase weights, nef_poly_weights), y [..][Cout_g / 2][2 T]; bit0 as above;
     *                  bias and stats only; followed by nef_poly_fwd_edge.
     *   pro_mode 4 (alone, wino == 3 only): phase-stacked input for the polyphase backward-data pass -- x is a full-resolution
     *                  tensor [..][Cin_g / 2][2 T]; reduction channel 2 c + p at position m is x[c][2 m + p] (see nef_poly_weights).
     * Zero padding is applied after the prologue.  in_scale must be NULL when pro_mode != 0. */
    const float* pro_a;
    const float* pro_b;
    int32_t pro_mode;
    int32_t pro_Bp;
    const uint64_t* rng_seed_dev;  /* NULL, or a device word added to rng_seed at run time (hipGraph replay: a captured
                                      launch freezes its arguments, the per-step seed must live in device memory) */
    int32_t wino;          /* 1: wp was packed with nef_pack_desc.wino 1 -- K == 3 through Winograd F(2,3), K == 7 through
                              F(2,4) + F(2,3) (2/3 resp. 9/14 of the multiplies; still fp32 multiplies and adds on the matrix cores, results differ
                              from the direct form by the rounding of the transforms).  2: packed with
                              wino 2 -- Winograd F(4,3) resp. F(4,4) + F(4,3): 1/2 resp. 13/28 of the multiplies.  Needs T even, T >= 128
                              (Cout_g % 128 == 0) or T >= 256 (Cout_g % 64 == 0), Cin_g % 16 == 0; K == 7: pro_mode 0.
                              3: packed with wino 3 -- the direct convolution on exact fp16 splits of both operands
                              (K == 1, 3 or 7, Cout_g % 64 == 0, Cin_g % 16 == 0, T even and >= 128; every epilogue option
                              incl. stats / bnb_slots; K == 7: pro_mode 0).  Short rows, 8 <= T <= 64 with T % 4 == 0
                              (K == 1 or 3): several samples per tile; then no prologue, in_scale, stats or bnb_slots. */
    float* stats;          /* NULL, or (wino == 2 only) the epilogue also leaves, per output channel and per 128-column slot
                              of a sample, the sum and the sum of squares of the final outputs of that slot:
                              stats[(ch * B * nslot + b * nslot + slot) * 2 + {0,1}], ch = g*Cout_g + co, nslot =
                              nef_conv_stats_slots(T, Cout_g) -- the train-mode BatchNorm statistics of the conv output
                              (model_nefnet.py:19,22) without a second pass over it; finished by nef_bn_stats_from_slots */
    /* BatchNorm-BACKWARD sums of the layer this (backward-data) launch propagates into, wino == 2 only, not together with
     * `stats`: with bnb_slots != NULL the epilogue also leaves, in the same slot layout, sum(g*m) and sum(g*m*xhat) of its
     * final outputs g, where m = [bnb_x*bnb_a + bnb_b > 0] and xhat = (bnb_x - bnb_mean)*bnb_invstd -- the reduction pass
     * of nef_bn_relu_bwd over (g, x), which then takes `slots` instead.  bnb_x: the BatchNorm input, dense
     * [B][G*Cout_g][T]; bnb_mean/invstd/a/b: [P][G*Cout_g], pass p = sample / bnb_Bp. */
    const float* bnb_x;
    const float* bnb_mean;
    const float* bnb_invstd;
    const float* bnb_a;
    const float* bnb_b;
    float* bnb_slots;
    int32_t bnb_Bp;
    int32_t bnb_up;        /* 1: a x2 linear upsampling (nn.Upsample, align_corners=False) sits between that BatchNorm's ReLU
                              and this launch's output: bnb_x is [B][G*Cout_g][T/2] and the sums are those of the
                              upsampling's adjoint (what nef_bn_relu_bwd form 2 reduces); T % 4 == 0 */
    float x_scale;         /* wino == 3 only: 0 (= 1) or an exact power of two the input is multiplied by before it is split into
                              fp16 terms and the accumulators are divided by again -- brings operands far from magnitude 1
                              (gradients) into fp16's range; the result is unchanged up to the split's rounding */
    int32_t reserved0;
    const float* x_amax;   /* wino == 3: NULL, or a device word holding the largest |input| (after in_scale / prologue) this call
                              site saw at its previous launch: when it is a positive finite number the input scale is derived
                              from it (-> [2^8, 2^9)) instead of x_scale -- the operand is then in fp16's range whatever its
                              magnitude, and the launch stays capturable (nothing is read back by the host) */
    float* x_amax_next;    /* wino == 3: NULL, or a device word (zeroed by the caller) this launch max-accumulates the largest
                              |input| of ITS operand into -- next launch's x_amax */
    int32_t* x_clamped;    /* wino == 3: NULL, or a device counter the launch adds 1 to (per wave) when an element of its operand is
                              still out of fp16's range AFTER the range rescue -- i.e. is not finite.  (A tile whose finite data does
                              not fit under the launch's scale -- the operand grew more than ~64x since x_amax was measured -- is
                              redone inside the launch with the scale its own data asks for; round 4 clamped it and counted it.) */
    const float* res_scale;   /* wino == 3, res != NULL: NULL, or a per-(sample, channel) factor on the residual,
                              y = conv + bias + res * res_scale[b*rs_bs + g*rs_gs + c] -- the residual of a block whose input is a
                              channel-scaled tensor (w_conv behind the theta scaling, codes/network/model_nefnet.py:122-124) read
                              from the UNSCALED tensor, with in_scale on the block's first conv: the scaled tensor is never written */
    int64_t rs_bs, rs_gs;
    const float* gate_rowscale;   /* wino == 3, gate != NULL: NULL, or a per-(sample, channel) factor on the gated output,
                              y = gate > 0 ? y * gate_scale * gate_rowscale[b*gr_bs + g*gr_gs + c] : 0 -- the backward of the same
                              channel scaling (nef_chscale_bwd's gx) taken in the epilogue of the block's last backward-data launch */
    int64_t gr_bs, gr_gs;
    int32_t stats_mode;    /* what `stats` receives: 0 = per-slot sum and sum of squares of the outputs; 1 (wino == 3, gate != NULL) =
                              per-slot sum of (ungated, unscaled output) x gate in word 0, 0 in word 1 -- nef_chscale_bwd's gs[b][c]
                              = sum_t gy x, finished by nef_slots_to_rows */
    int32_t reserved1;
} nef_conv_args;

/* y = epilogue(conv(x * in_scale, wp) + bias + res).  Also the bwd-data pass (pack with transpose_flip=1,
 * swap Cin_g/Cout_g). */
int nef_conv_fwd(const nef_conv_args* a, nef_stream_t stream);
/* The same launch with one promise added: the operand x, after in_scale, is EXACTLY zero at every t >= live[b*G + g] + live_add
 * (live: device int32 [B][G], e.g. nef_live_extent's table; live_add: what the convs between the stem and this operand widened it
 * by).  The plain split-fp16 forms (wino 3, pro_mode 0, T >= 128; K = 1, 3, 7) then skip the main loop of every 256-column tile
 * whose staged window t0 - (K-1)/2 .. lies behind that bound: no operand loads, no matrix instructions, no rescue pass.  The
 * epilogue runs unchanged on zero accumulators -- bias, residual, ReLU, dropout, gate, statistics, x_amax_next and every output
 * store -- so the result is what nef_conv_fwd gives, bit for bit, with finite weights (products of zeros accumulate to +0).
 * A non-finite weight would have turned those zeros into NaN; such a step is already broken and the live tiles still report it.
 * Every other form (other wino, prologues, short rows) ignores the table and runs as nef_conv_fwd.  A promise that does not hold
 * gives wrong results silently: derive it from a measured table and a chain of bias-free convs only. */
int nef_conv_fwd_live(const nef_conv_args* a, const int32_t* live, int32_t live_add, nef_stream_t stream);
/* Zero-fill exit.  A dead tile of such a launch (its window behind the bound as above) stores +0.0 to
 * its outputs and leaves -- no operand, table, LDS or barrier -- when the launch says that the epilogue maps a zero accumulator to
 * zero at every output of the tile: no bias, no statistics (stats / bnb_slots NULL; a stats_mode 1 launch therefore keeps the full
 * epilogue), and no residual -- or, through nef_conv_fwd_live_res, a residual with a promise of its own: a->res (after res_scale) is
 * exactly zero at every t >= live[b*G + g] + res_add, and the tile qualifies only if t0 >= live + res_add.  ReLU, dropout and the
 * gate keep zeros and need no condition; where a negative gate scale would have written -0.0 this path writes +0.0 (equal as
 * numbers, and a later conv's sums do not tell them apart).  x_amax_next and x_clamped need nothing: a dead tile's magnitude is 0.
 * A dead tile that does not qualify runs the path above.  nef_conv_fwd_live_res requires a->res; everything else as
 * nef_conv_fwd_live.  An addition: the ABI number stays, a binding finds a library without it by the missing symbol. */
int nef_conv_fwd_live_res(const nef_conv_args* a, const int32_t* live, int32_t live_add, int32_t res_add, nef_stream_t stream);
/* sizeof(nef_conv_args) as the library was built: a binding checks its mirror of the struct against it. */
size_t nef_conv_args_bytes(void);

/* gw[g*Cog+co][ci][k] = sum_{b,t} gy[b][g][co][t] * x'[b][g][ci][t+k-pad], x' = prologue(x) * in_scale.  gw is overwritten.
 * One struct describes the call, as nef_conv_args does for the forward / backward-data convolutions (same names, same meaning).
 * Fields a form does not use are ignored (forms 0 and 4: x_scale, gy_scale, the amax words and `clamped`), so one struct can be
 * handed from form 3 to form 0 as it is. */
typedef struct nef_bww_args {
    const float* x;        /* input; element (b, g, ci, t) at x + b*x_bs + g*x_gs + ci*T + t (half resolution, T/2, with pro_mode bit1) */
    const float* gy;       /* output gradient; element (b, g, co, t) at gy + b*gy_bs + g*gy_gs + co*T + t */
    float* gw;             /* [G*Cout_g][Cin_g][K], torch layout */
    void* ws;              /* ws_bytes >= nef_conv_bwd_weight_ws_bytes(args) bytes of scratch: the split partial sums, added up in a
                              fixed order (deterministic) */
    const float* in_scale; /* NULL, or per (sample, input channel) factor at in_scale + b*sc_bs + g*sc_gs + ci; only with pro_mode 0 */
    const float* pro_a;    /* the input prologue of nef_conv_args (pro_mode / pro_a / pro_b / pro_Bp), recomputed while staging x: */
    const float* pro_b;    /* bit0 needs pro_a, pro_b and pro_Bp > 0; without bit0 pro_Bp <= 0 means 1 */
    /* Form 3 only.  x_amax / gy_amax: NULL, or device words with the largest |operand| the call site saw before -- when positive and
     * finite the scales are derived from them instead of x_scale / gy_scale; x_amax_next / gy_amax_next: both NULL, or device words
     * this launch max-accumulates its operands' magnitudes into; clamped: NULL, or a device counter incremented when a scaled
     * operand element had to be clamped at fp16's range (see nef_conv_args.x_clamped). */
    const float* x_amax;
    const float* gy_amax;
    float* x_amax_next;
    float* gy_amax_next;
    int32_t* clamped;
    size_t ws_bytes;
    int64_t x_bs, x_gs, gy_bs, gy_gs, sc_bs, sc_gs;
    int32_t B, T, G, Cin_g, Cout_g, K;
    int32_t pro_mode;      /* 0..3 as in nef_conv_args (K == 3 only); form 3 also takes bit 2 (4 / 5, no upsampling bit, Cout_g % 128
                              == 0: the producer / consumer form): the window's columns -1 and T hold x'[0] and x'[T-1] instead of
                              zeros (the polyphase weight gradient) */
    int32_t pro_Bp;
    int32_t form;          /* which kernel family; anything else: NEF_E_UNSUPPORTED.
                            * 0: the direct fp32 kernel.  K == 1, 3 or 7; a prologue (pro_mode 1..3) only with K == 3 and in_scale ==
                            *    NULL, T even with the upsampling bit.
                            * 4: the TRANSPOSED Winograd algorithm (in_scale or the input prologue); fp32 multiplies and adds on the
                            *    matrix cores, results differ from the direct form by the rounding of the transforms.  Needs T even and
                            *    T >= 64; K == 7: pro_mode 0.
                            *      K == 3: transposed F(3,4), 6 multiplies per four columns -- 1/2 of the direct form's; transform entries
                            *              up to 8 and 1/24 (the F(4,3) matrices of the forward kernels, roles exchanged): measured
                            *              rounding 1..6x the direct form's.
                            *      K == 7: the taps split 4 + 3 across TWO launches, transposed F(4,4) + transposed F(3,4): 13 multiplies
                            *              per 8 columns (direct: 28).
                            *    Which kernel runs: the (gy, x) tiles are streamed by LDS-DMA through a ring of LDS buffers
                            *    (csrc/conv_bww_glds.hip) when in_scale == NULL, both channel counts are multiples of 64, T >= 64, T % 4
                            *    == 0 if pro_mode has the upsampling bit, not both prologue bits at once, and at most 8 BatchNorm
                            *    passes (B / pro_Bp); otherwise the register-staged kernel of csrc/conv_mfma.hip.  Same arithmetic and
                            *    partial-sum layout; the two differ only by the summation order across splits.  The kernel never reads
                            *    outside [x, x + (B-1)*x_bs + (G-1)*x_gs + Cin_g*T) resp. the same extent of gy.  (ABI <= 11 also had
                            *    nef_conv_bwd_weight_wino, the transposed F(3,2): removed, this form covers every shape it took.)
                            * 3: exact fp16 splits of BOTH operands (csrc/conv_h2w.hip; the arithmetic of the wino = 3 pack / conv
                            *    args wino = 3, the same family: gy = gh + gl, X = xh + xl, three fp16 matrix instructions per product,
                            *    fp32 accumulation): fp32-class results (closer to fp64 than the transposed-Winograd forms) at 3/16 of
                            *    the fp32 matrix instructions' pipe time.  K == 3 (any pro_mode) or K == 7 (pro_mode 0), T even and
                            *    >= 64, both channel counts multiples of 64; in_scale only with pro_mode 0. */
    float x_scale;         /* form 3: 0 (= 1) or the exact powers of two the operands are multiplied by before they are split (their */
    float gy_scale;        /* product is divided out) */
    int32_t reserved0;
} nef_bww_args;

int nef_conv_bwd_weight(const nef_bww_args* a, nef_stream_t stream);
/* Form 3 with one promise added: every product of a (sample b, 64-column tile t0) item with t0 >= live[b*G + g] + live_add is zero
 * (live: device int32 [B][G], nef_live_extent's table).  The caller picks live_add for whichever operand is zero-tailed: the
 * gradient's bound (gy exactly zero at t >= bound), or the input's bound + (K-1)/2 (the item's window starts at t0 - (K-1)/2).
 * The shares of the (sample, tile) sequence keep their boundaries in the FULL item space; inside each share the dead items are left
 * out, in order -- a dead item only adds products of zeros (+0), so every partial sum and gw keep nef_conv_bwd_weight's bits (finite
 * operands; a NaN or Inf opposite a promised zero would have made a NaN: such a step is already broken).  x_amax_next / gy_amax_next
 * are taken over the live items: the words (and with them the next launch's scales and the
 * share's rescue decision) are nef_conv_bwd_weight's only when BOTH operands are zero in the dead items; with a lone promised
 * operand the other one's word covers its live part only.  A caller that needs the words unchanged -- the train step does: they
 * set the next step's scales -- hands the promise over only where both operands carry the tail (engine.block_bwd).  A small launch in
 * front builds the item tables in the workspace, behind the partial sums: nef_conv_bwd_weight_ws_bytes counts them in.  The
 * producer / consumer kernel without a prologue (Cout_g % 128 == 0, pro_mode 0) skips; the other kernels of the form run as before. */
int nef_conv_bwd_weight_live(const nef_bww_args* a, const int32_t* live, int32_t live_add, nef_stream_t stream);
/* Reads form, B, T, G, Cin_g, Cout_g, K only; 0: unsupported shape or form.  Forms 0 and 4: the split bound of the prologue-free
 * direct plan (no plan with a prologue or a Winograd form has more splits); form 3: sized for whichever tile form the launch's
 * prologue mode takes (the largest over the modes). */
size_t nef_conv_bwd_weight_ws_bytes(const nef_bww_args* a);
/* sizeof(nef_bww_args) as the library was built: a binding checks its mirror of the struct against it. */
size_t nef_bww_args_bytes(void);

/* Heavy-tail census of one split-fp16 operand (ops._note_tail, once per call site, at its measuring launch; no counterpart in the
 * reference, whose fp32 convs keep every element's bits).  The operand is described as the launch reads it: the view
 * x[b][g][c][t] at x + b x_bs + g x_gs + c T + t; pro_mode bit 0 applies the affine + ReLU prologue max(fma(x, a, b), 0), a / b
 * [pass = b / pro_Bp][g Cg + c]; in_scale (NULL or [b sc_bs + g sc_gs + c]) multiplies after it.  With the x2 upsampling bit (2)
 * the view is the half-resolution input and its values are counted (the interpolated ones are blends of them), while `amax` is the
 * interpolated operand's, which can be smaller than the largest half-resolution value (v / amax may exceed 1: no count changes);
 * bits 2 / 3 add no values.  `amax`: device word with the operand's largest magnitude (the measuring launch's slot).  Counted: nonzero elements, and
 * those below window x amax; energies: the sums of (v / amax)^2 over both sets (fp32 per wave and row, fp64 across rows).  flag =
 * (n_small / n_nonzero > frac).  Two launches (block partials in ws, one fixed-order combine): nothing synchronises, results are
 * bitwise reproducible.  site_flag: NULL, or a device word set to 1 when flag is; tail_stat: NULL, or two device words that keep
 * the largest count / energy fraction seen.  ws: nef_h2_tail_census_ws_bytes(B, G, Cg) bytes. */
typedef struct nef_h2_tail_census_out {
    uint64_t n_nonzero, n_small;
    double e_small, e_total;
    float frac_count, frac_energy;
    int32_t flag, reserved;
} nef_h2_tail_census_out;
size_t nef_h2_tail_census_ws_bytes(int B, int G, int Cg);
int nef_h2_tail_census(const float* x, int64_t x_bs, int64_t x_gs, int B, int G, int Cg, int T, const float* in_scale, int64_t sc_bs,
                       int64_t sc_gs, const float* pro_a, const float* pro_b, int pro_mode, int pro_Bp, const float* amax, float window,
                       float frac, void* ws, size_t ws_bytes, nef_h2_tail_census_out* out, int32_t* site_flag, float* tail_stat,
                       nef_stream_t stream);
/* gw [G Cout_g][Cin_g][3] += the row-end terms by which a K = 3 weight gradient over a window continued with x'[0] / x'[T-1] at both
 * row ends (nef_bww_args form 3, pro_mode bit 2) differs from the zero-padded one: gw[r][ci][0] += sum_b gy[b][r][0] xedge[b][ci][0],
 * gw[r][ci][2] += sum_b gy[b][r][T-1] xedge[b][ci][1]; xedge [B][G Cin_g][2] = x' (the prologue's output) at both row ends, as
 * nef_poly_fwd_edge writes it.  After an fp32 weight gradient (nef_bww_args form 0) with pro_mode & 1 this gives the polyphase
 * phase-weight gradient that nef_poly_wgrad_fold takes (the fp32 route of a heavy-tailed site).  Cout_g % 16 == 0; samples summed
 * in order, no atomics. */
int nef_bwd_weight_clamp_ends(const float* xedge, const float* gy, int64_t gy_bs, int64_t gy_gs, float* gw, int B, int T, int G,
                              int Cin_g, int Cout_g, nef_stream_t stream);

/* out[c] = sum_{b,t} x[b][c][t] (bias gradients).  ws: nef_chan_sum_ws_bytes(C). */
size_t nef_chan_sum_ws_bytes(int C);
int nef_chan_sum(const float* x, float* out, void* ws, size_t ws_bytes, int B, int C, int T, nef_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ConvTranspose1d(k=2, s=2, groups=G, 128 -> 64 per group, bias).  codes/network/model_nefnet.py:96-97.
 *   x [B][G*Cig][T], w [G*Cig][Cog][2], bias [G*Cog], y [B][G*Cog][2T]. */
int nef_convt2_fwd(const float* x, const float* w, const float* bias, float* y, int B, int G, int Cig, int Cog,
                   int T, nef_stream_t stream);
int nef_convt2_bwd_data(const float* gy, const float* w, float* gx, int B, int G, int Cig, int Cog, int T,
                        nef_stream_t stream);
/* The same op through the matrix cores: a grouped 1x1 conv onto m = co*2+j (nef_conv_fwd, K=1, weights
 * nef_group_transpose'd to [G][2Cog][Cig]) + these layout passes:
 *   nef_group_transpose    : out[g][c][r] = in[g][r][c]                     (weights both ways: the op is an involution)
 *   nef_convt2_interleave  : y[b][c][2t+j] = yq[b][2c+j][t] + bias[c]       (bias may be NULL), C = G*Cog
 *   nef_convt2_deinterleave: gyq[b][2c+j][t] = gy[b][c][2t+j] */
int nef_group_transpose(const float* in, float* out, int G, int R, int Cn, nef_stream_t stream);
int nef_convt2_interleave(const float* yq, const float* bias, float* y, int B, int C, int T, nef_stream_t stream);
int nef_convt2_deinterleave(const float* gy, float* gyq, int B, int C, int T, nef_stream_t stream);
size_t nef_convt2_bwd_weight_ws_bytes(int G, int Cig, int Cog);
int nef_convt2_bwd_weight(const float* x, const float* gy, float* gw, float* gb, void* ws, size_t ws_bytes, int B,
                          int G, int Cig, int Cog, int T, nef_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Angular encoding + Linear(12 -> O).  codes/network/utils/theta_encoder.py:13-29 with
 * model_nefnet.py:76-77,121,164,183.   theta [N][2], W [O][12], bias [O], y [N][O]. */
int nef_theta_mlp_fwd(const float* theta, const float* W, const float* bias, float* y, int N, int O,
                      nef_stream_t stream);
int nef_theta_mlp_bwd(const float* theta, const float* gy, float* gW, float* gb, int N, int O, nef_stream_t stream);
/* enc [N][12] only (test hook for the encoding itself). */
int nef_theta_encode(const float* theta, float* enc, int N, nef_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-(sample, channel) scaling.  model_nefnet.py:122-123 (lead latents x mlp1) and :166,170,174,186.
 *   y[b][c][t] = x[b][c][t] * s[b*s_bs + c];  bwd: gx = gy * s, gs[b][c] = sum_t gy * x (gs dense [B][C]). */
int nef_chscale_fwd(const float* x, const float* s, int64_t s_bs, float* y, int B, int C, int T, nef_stream_t stream);
/* relu_x != 0: x is a ReLU output; gx is additionally masked with x > 0 (the gate its producer's backward starts with). */
int nef_chscale_bwd(const float* gy, const float* x, const float* s, int64_t s_bs, float* gx, float* gs, int B,
                    int C, int T, int relu_x, nef_stream_t stream);

/* out = g * scale * (ref > 0)   (ReLU / dropout back-propagation gate), n elements. */
int nef_gate(const float* g, const float* ref, float* out, float scale, int64_t n, nef_stream_t stream);
/* out = a + b, n elements. */
int nef_add(const float* a, const float* b, float* out, int64_t n, nef_stream_t stream);
/* Time-window copy of a grouped view: dst [B][G*Cg][W] dense <- src(b,g,c, t0 + w)  (src strides x_bs / x_gs, rows T). */
int nef_window_crop(const float* src, int64_t x_bs, int64_t x_gs, float* dst, int B, int G, int Cg, int T, int t0, int W,
                    nef_stream_t stream);
/* Inverse: dst(b,g,c,t) = (t0 <= t < t0+W) ? src[b][g*Cg+c][t-t0] : 0 over the whole grouped view (zero fill). */
int nef_window_scatter(const float* src, float* dst, int64_t y_bs, int64_t y_gs, int B, int G, int Cg, int T, int t0,
                       int W, nef_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ROI ops.  rois: int64 [B][7][2] in input-sample units; latent index = roi * 0.25 (model_nefnet.py:136,143).
 * nef_roi_align_*: codes/network/utils/roi_pooling_1d.py:38-69 with the reference's actual semantics
 *   (grid x addresses the size-1 axis).  z [B][C][T] -> out [B][C][7][16].  Only the two middle rows of
 *   time are ever read, so z / gz may store just a window: zT samples per row starting at time t_off (zT=T, t_off=0
 *   for a full tensor); the window must contain rows (T-1)/2 and (T-1)/2+1.
 * nef_roi_unpool_*: roi_pooling_1d.py:72-99.  zseg [B][C][7][32] -> out [B][C][T].
 *   status (int32[1], may be NULL): set to 1 if a sample's segment lengths are negative or do not sum to T. */
int nef_roi_align_fwd(const float* z, const int64_t* rois, float* out, int B, int C, int T, int zT, int t_off,
                      nef_stream_t stream);
int nef_roi_align_bwd(const float* gout, const int64_t* rois, float* gz, int B, int C, int T, int zT, int t_off,
                      nef_stream_t stream);
int nef_roi_unpool_fwd(const float* zseg, const int64_t* rois, float* out, int32_t* status, int B, int C, int T,
                       nef_stream_t stream);
int nef_roi_unpool_bwd(const float* gout, const int64_t* rois, float* gzseg, int B, int C, int T,
                       nef_stream_t stream);
/* seg_start/seg_len int64 [B][7]: the integer bookkeeping of roi_pooling_1d.py:82-92 (bit-exact test hook). */
int nef_roi_segment_table(const int64_t* rois, int64_t* seg_start, int64_t* seg_len, int B, nef_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Lead mean / Standin shuffle / query scaling.  model_nefnet.py:146-176.
 *   z1, z2r [B][128V][T]; latent [B][256][T] = cat(mean_v z1, mean_v z2r);
 *   q [B][256];  D [3][B][256][T]:  D0 = q*latent, D1 = q*cat(z1[c1], z2mean), D2 = q*cat(z1mean, z2r[c2]).
 *   choice_dev: NULL, or device int32[2] = {c1, c2} that overrides the arguments (hipGraph replay). */
int nef_lead_mean(const float* z1, const float* z2r, float* latent, int B, int V, int T, nef_stream_t stream);
int nef_mix_fwd(const float* latent, const float* z1, const float* z2r, const float* q, float* D, int B, int V,
                int T, int c1, int c2, const int32_t* choice_dev, nef_stream_t stream);
int nef_mix_bwd(const float* gD, const float* latent, const float* z1, const float* z2r, const float* q, float* gz1,
                float* gz2r, float* gq, int B, int V, int T, int c1, int c2, const int32_t* choice_dev, int relu_z1, int up,
                int shared, nef_stream_t stream);
/* relu_z1 != 0: z1 is a ReLU output; gz1 is additionally masked with z1 > 0.
 * up != 0: gD is the gradient wrt the x2-UPSAMPLED decoder input, [..][256][2T] (what the first decoder conv's backward-data
 *   writes); the upsampling adjoint (nef_upsample2_bwd) is taken while reading it.  Any T >= 1, as nef_upsample2_bwd.
 * shared != 0: gD is the two-pass gradient wrt D2 of nef_mix_fwd_shared (below), [2B][256][T] or, with `up`, [2B][256][2T],
 *   instead of the three-pass [3B][256][..].  T > 1. */

/* Shared first decoder conv (train step): the three decoder inputs of model_nefnet.py:159-176 are
 * q*cat(z1m|z2m), q*cat(z1[c1]|z2m), q*cat(z1m|z2r[c2]) and decoder.1.double_conv.0 is linear in the two channel halves,
 * so each distinct half goes through its half of the conv once (4 half-convs instead of 6):
 *   nef_mix_fwd_shared   : D2 [2B][256][T] = (q*cat(z1m|z2m) | q*cat(z1[c1]|z2r[c2]))
 *   (grouped conv, G = 2, on D2 with the weight regrouped to [2*Cout][Cin/2][3] -> P2 [2B][2C][L])
 *   nef_pass_combine_fwd : c1[p][b][c] = P2 A-half[ia(p)] + P2 B-half[ib(p)] + bias[c],  (ia,ib) = (m,m),(pick,m),(m,pick)
 *   nef_pass_combine_bwd : its adjoint, gc1 [3B][C][L] -> gP2 [2B][2C][L]
 *   nef_mix_bwd, shared = 1: the adjoint of nef_mix_fwd_shared, from the two-pass gradient wrt the upsampled D2 (up = 1) or wrt
 *                          D2 itself (up = 0: what the polyphase backward-data pass leaves). */
int nef_mix_fwd_shared(const float* latent, const float* z1, const float* z2r, const float* q, float* D2, int B, int V,
                       int T, int c1, int c2, const int32_t* choice_dev, nef_stream_t stream);
/* nef_lead_mean + nef_mix_fwd_shared in one pass over z1 / z2r (the picked lead is one of the rows being averaged):
 * bit-identical latent and D2, 0.65 GB less traffic per step at config 2. */
int nef_lead_mean_mix_shared(const float* z1, const float* z2r, const float* q, float* latent, float* D2, int B, int V,
                             int T, int c1, int c2, const int32_t* choice_dev, nef_stream_t stream);
/* The same two outputs straight from the segment tensor z2b [B][128V][7][32] of nef_roi_unpool_fwd's input: the un-pooled tensor
 * z2r is never written.  latent and D2 are bit-identical to nef_roi_unpool_fwd followed by nef_lead_mean_mix_shared, `status` is
 * raised as nef_roi_unpool_fwd raises it.  The z1 half runs nef_lead_mean_mix_shared's kernels on the rows c < 128; the z2 half holds
 * the V leads' segment samples of a (sample, channel) row on chip, evaluates the resampling taps once per output position and forms
 * mean and pick there.  1 <= V <= NEF_UNPOOL_MIX_MAX_V. */
#define NEF_UNPOOL_MIX_MAX_V 12
int nef_lead_mean_mix_unpool(const float* z1, const float* z2b, const int64_t* rois, const float* q, float* latent, float* D2,
                             int32_t* status, int B, int V, int T, int c1, int c2, const int32_t* choice_dev, nef_stream_t stream);
/* Its adjoint: nef_mix_bwd(shared = 1, up = 0) followed by nef_roi_unpool_bwd without the gradient gz2r between them.
 * gD [2B][256][T], latent [B][256][T]; gz1 [B][128V][T], gz2b [B][128V][7][32] and gq [B][256] are bit-identical to the two calls
 * (the z2 half deals a row's positions to the lanes as the nef_mix_bwd kernel of the same shape does, so gq adds in the same order).  Of the V gradient rows of a (sample, channel) only two
 * differ -- the picked lead's and everyone else's -- so the gather transpose runs twice per row, not V times; the picked lead's
 * un-pooled value that gq needs is rebuilt from z2b.  2 <= T <= NEF_UNPOOL_MIX_MAX_T (two gradient rows per wave in LDS). */
#define NEF_UNPOOL_MIX_MAX_T 1936
int nef_mix_bwd_unpool(const float* gD, const float* latent, const float* z1, const float* z2b, const int64_t* rois, const float* q,
                       float* gz1, float* gz2b, float* gq, int B, int V, int T, int c1, int c2, const int32_t* choice_dev, int relu_z1,
                       nef_stream_t stream);
/* nef_mix_bwd_unpool that also leaves gz1_chan_sum [128V] = sum_{b,t} gz1[b][c][t] of the gz1 it stores (after the relu_z1 mask): the bias
 * gradient of the residual 1x1 conv that reads gz1, without reading gz1 back.  gz1, gz2b and gq are bit-identical to nef_mix_bwd_unpool.
 * Where the 16-byte pair kernel runs (T % 4 == 2, T >= 8, 16-byte aligned tensors) and V <= 4 it adds what it stores, in fp64 from the first
 * element, per (sample, lead, channel) row, and the rows are summed over the samples in a fixed order; *in_kernel (may be NULL) is then
 * 1.  Otherwise the sum is taken by nef_chan_sum over the stored gz1 and *in_kernel is 0.  ws: nef_mix_bwd_unpool_rs_ws_bytes(B, V). */
int nef_mix_bwd_unpool_rs(const float* gD, const float* latent, const float* z1, const float* z2b, const int64_t* rois, const float* q,
                          float* gz1, float* gz2b, float* gq, float* gz1_chan_sum, void* ws, size_t ws_bytes, int* in_kernel, int B, int V,
                          int T, int c1, int c2, const int32_t* choice_dev, int relu_z1, nef_stream_t stream);
size_t nef_mix_bwd_unpool_rs_ws_bytes(int B, int V);
int nef_pass_combine_fwd(const float* P2, const float* bias, float* c1, int B, int C, int L, nef_stream_t stream);
/* nef_pass_combine_fwd that also leaves the train-mode BatchNorm statistics of its output (3 passes of B samples; same
 * outputs as nef_bn_train_stats(c1, ..., P = 3, Bp = B, ...), running statistics updated pass by pass): saves the separate
 * statistics pass over c1.  ws: nef_pass_combine_stats_ws_bytes(B, C). */
size_t nef_pass_combine_stats_ws_bytes(int B, int C);
int nef_pass_combine_fwd_stats(const float* P2, const float* bias, float* c1, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, float* mean, float* invstd, float* a, float* b,
                               void* ws, size_t ws_bytes, int B, int C, int L, float eps, float momentum,
                               int64_t* num_batches_tracked, nef_stream_t stream);
int nef_pass_combine_bwd(const float* gc1, float* gP2, int B, int C, int L, nef_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Decoder pieces.  model_nefnet.py:10-27,101-107.
 * Upsample(scale 2, linear, align_corners=False): x [N][Tin] rows -> y [N][2Tin]. */
int nef_upsample2_fwd(const float* x, float* y, int64_t N, int Tin, nef_stream_t stream);
int nef_upsample2_bwd(const float* gy, float* gx, int64_t N, int Tin, nef_stream_t stream);

/* BatchNorm1d, training mode, P independent passes stacked along batch (x [P*Bp][C][L]).
 * nef_bn_train_stats: per (pass, channel) batch mean / biased var -> mean, invstd [P][C], the affine
 *   a = gamma*invstd, b = beta - mean*a [P][C]; then updates running_mean/var sequentially over passes with
 *   momentum (unbiased var), exactly as P successive module calls would.
 * nef_bn_eval_affine: a = gamma/sqrt(rv+eps), b = beta - rm*a  [C].
 * nef_affine_relu_fwd: y = max(0, x*a[p][c] + b[p][c]).
 * nef_bn_relu_bwd: the backward of BatchNorm + ReLU, one nef_bn_bwd_args struct per call (below). */
size_t nef_bn_ws_bytes(int P, int C);
/* Slots per sample of nef_conv_args.stats (0: the F(4,3) kernel does not take this shape), and the statistics pass that
 * replaces nef_bn_train_stats when the producing conv left them: same outputs (fp64 from the slot sums on, fixed
 * order), x is not read.  slots: [C][P*Bp*nslot][2] floats.  ws: nef_bn_ws_bytes(P, C). */
int nef_conv_stats_slots(int T, int Cout_g);
int nef_bn_stats_from_slots(const float* slots, int nslot, const float* gamma, const float* beta, float* running_mean,
                            float* running_var, float* mean, float* invstd, float* a, float* b, void* ws,
                            size_t ws_bytes, int P, int Bp, int C, int L, float eps, float momentum,
                            int64_t* num_batches_tracked, nef_stream_t stream);
int nef_bn_train_stats(const float* x, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, float* mean, float* invstd, float* a, float* b, void* ws, size_t ws_bytes,
                       int P, int Bp, int C, int L, float eps, float momentum, int64_t* num_batches_tracked,
                       nef_stream_t stream);
/* (round 6) num_batches_tracked: NULL, or the BatchNorm's int64 counter, incremented by the number of passes P by the same launch
 * that updates the running statistics (nn.BatchNorm1d in train mode, codes/network/model_nefnet.py:19,22) -- in all three entry
 * points above (nef_pass_combine_fwd_stats: P = 3). */
int nef_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float* a, float* b, int C, float eps, nef_stream_t stream);
/* Eval-mode BN folded into the preceding conv (inference sweep): w_out[co][:] = a[co]*w[co][:], bias_out = a*bias + b;
 * w [Cout][inner]. */
int nef_fold_bn(const float* w, const float* bias, const float* a, const float* b, float* w_out, float* bias_out,
                int Cout, int inner, nef_stream_t stream);
int nef_affine_relu_fwd(const float* x, const float* a, const float* b, float* y, int P, int Bp, int C, int L,
                        nef_stream_t stream);
/* BatchNorm + ReLU backward.  Given the gradient wrt the ReLU output and x (pre-BN), writes gx, ggamma[C], gbeta[C] and, when asked,
 * the per-channel sum of gx, all from one reduction and one apply pass.  One struct describes the call; `form` picks the kernel
 * family.  A combination no kernel serves (an unknown form, phase_major on forms 1 or 2, slots on form 1, P != 3 on form 3, a
 * gradient pointer the form does not read) is NEF_E_UNSUPPORTED, never ignored. */
typedef struct nef_bn_bwd_args {
    const float* g;        /* the incoming gradient.  Forms 0 and 3: gy [P*Bp][C][L], wrt the ReLU output.  Form 2: gu [P*Bp][C][2L], wrt
                              nn.Upsample(x2)(ReLU(BN(x))) (model_nefnet.py:104).  Form 1: NULL */
    const float* gout;     /* form 1 only (NULL otherwise): the gradient wrt the network output [P*Bp][L], */
    const float* out;      /* that output (the sigmoid's), [P*Bp][L], */
    const float* wout;     /* and the last conv's weight [1][C][3] */
    const float* x;        /* the BatchNorm input [P*Bp][C][L] */
    const float* mean;     /* [P][C], as nef_bn_train_stats left them */
    const float* invstd;
    const float* a;
    const float* b;
    float* gx;             /* [P*Bp][C][L]; with phase_major [P*Bp][2C][L/2].  Form 3 writes gP2 [2Bp][2C][L] here instead, with
                              phase_major [2Bp][4C][L/2] (only gx's per-channel sum is kept) */
    float* ggamma;         /* [C] */
    float* gbeta;          /* [C] */
    float* gx_chan_sum;    /* NULL, or [C]: sum_{b,t} gx, the bias gradient of the conv that feeds this BatchNorm */
    const float* slots;    /* NULL, or the sums the conv that produced g left in its epilogue (nef_conv_args.bnb_slots): the
                              reduction pass over (g, x) is then skipped.  Not with form 1 */
    void* ws;              /* ws_bytes >= nef_bn_bwd_ws_bytes(args) bytes of scratch */
    size_t ws_bytes;
    int32_t P, Bp, C, L;   /* P independent passes of Bp samples stacked along batch */
    int32_t nslot;         /* with slots: nef_conv_stats_slots of the producing launch; > 0, Bp*nslot <= INT_MAX */
    int32_t form;          /* 0: plain.  Any L; the row kernel when L % 4 == 0 and P*Bp*C <= INT_MAX, else the element kernel.
                            * 1: fed straight from the last conv's output gradient: the [N][C][L] input gradient of Conv1d(C->1) (what
                            *    nef_outconv_bwd_data would write) is rebuilt on the fly from go = gout*out*(1-out)/3, so it is never
                            *    materialised.  Same results as nef_outconv_bwd_data + form 0.  L % 4 == 0, P*Bp*C <= INT_MAX.
                            * 2: g at TWICE the length; the upsampling adjoint (nef_upsample2_bwd) is taken while reading.  L % 4 == 0,
                            *    L >= 8, P*Bp*C <= INT_MAX.
                            * 3: form 0 with P == 3 followed by nef_pass_combine_bwd in one pass.  Bp*C <= INT_MAX. */
    int32_t phase_major;   /* forms 0 and 3: row r of the output is written as the two half-length rows 2 r (even positions) and
                              2 r + 1 (odd positions) -- the operand of the polyphase backward passes (below).  Form 0: L % 4 == 0
                              and P*Bp*C <= INT_MAX; form 3: L % 2 == 0 */
    int32_t reserved0;
} nef_bn_bwd_args;

int nef_bn_relu_bwd(const nef_bn_bwd_args* a, nef_stream_t stream);
/* Reads form, P, Bp, C, L only; 0: an unknown form or a non-positive size. */
size_t nef_bn_bwd_ws_bytes(const nef_bn_bwd_args* a);
/* sizeof(nef_bn_bwd_args) as the library was built: a binding checks its mirror of the struct against it. */
size_t nef_bn_bwd_args_bytes(void);
/* nef_bn_relu_bwd form 1 whose sums pass also leaves the gradients of the last Conv1d(C->1, k3, p1, bias) (model_nefnet.py:106,168):
 * gwout [1][C][3] and gbout [1], the outputs of nef_outconv_bwd_weight with x' = max(0, x*a + b), formed from the go values and the
 * x*a + b the pass already holds, so the [P*Bp][C][L] tensor is not streamed a third time.  gx, ggamma, gbeta and gx_chan_sum are
 * bit-identical to nef_bn_relu_bwd; gwout / gbout add in fp32 inside a lane's share of one sample row and in fp64, in a fixed order,
 * from there on.  Any form but 1 is NEF_E_UNSUPPORTED.  ws2: nef_bn_relu_bwd_outconv_w_ws_bytes (0 for a form other than 1), apart from
 * a->ws. */
int nef_bn_relu_bwd_outconv_w(const nef_bn_bwd_args* a, float* gwout, float* gbout, void* ws2, size_t ws2_bytes, nef_stream_t stream);
size_t nef_bn_relu_bwd_outconv_w_ws_bytes(const nef_bn_bwd_args* a);

/* Final Conv1d(64->1,k3,p1,bias) + sigmoid(x/3).  model_nefnet.py:106,168.
 *   x [N][C][L], w [1][C][3], bias [1], out [N][L].
 * a, b: both NULL, or x is the pre-BatchNorm tensor and x' = max(0, x*a[p][c] + b[p][c]), p = n / Bp, is applied on the fly. */
int nef_outconv_fwd(const float* x, const float* a, const float* b, int Bp, const float* w, const float* bias,
                    float* out, int N, int C, int L, nef_stream_t stream);
int nef_outconv_bwd_weight(const float* gout, const float* out, const float* x, const float* a, const float* b, int Bp,
                           float* gw, float* gb, void* ws, size_t ws_bytes, int N, int C, int L, nef_stream_t stream);
int nef_outconv_bwd_data(const float* gout, const float* out, const float* w, float* gx, int N, int C, int L,
                         nef_stream_t stream);
size_t nef_outconv_bwd_weight_ws_bytes(int C);

/* ---------------------------------------------------------------------------------------------
 * Loss.  codes/network/loss/losses.py:21-50 (+ solver.py:185-186 noise):
 *   l1 = mean|sg(pred)-pred_p|, l2 = mean|sg(pred)-pred_l|, l3 = mean|pred-target| (or squared, reg_l2),
 *   losses[4] = {f0*l1 + f1*l2 + f2*l3, f0*l1, f1*l2, f2*l3};  use_mask bit i enables term i+1.
 * bwd: gradients wrt pred (term 3 only), pred_p, pred_l scaled by gscale (d loss). */
size_t nef_loss_ws_bytes(void);
int nef_loss_fwd(const float* pred, const float* pred_p, const float* pred_l, const float* target, float* losses,
                 void* ws, size_t ws_bytes, int64_t n, float f0, float f1, float f2, int reg_l2, int use_mask,
                 nef_stream_t stream);
int nef_loss_bwd(const float* pred, const float* pred_p, const float* pred_l, const float* target,
                 const float* gscale /* device scalar */, float* g_pred, float* g_p, float* g_l, int64_t n, float f0,
                 float f1, float f2, int reg_l2, int use_mask, nef_stream_t stream);
/* The same two with cfg.DATA.noise (codes/solver/solver.py:185-186, `out = out + noise`): noise is NULL or n floats in pred's layout,
 * and every term and gradient is taken at pred[i] + noise[i] (one fp32 add; the Standin terms compare against the noisy prediction
 * as well, losses.py:34-38).  NULL noise: the entries above, bit for bit -- those are these with noise = NULL. */
int nef_loss_noise_fwd(const float* pred, const float* pred_p, const float* pred_l, const float* target,
                       const float* noise, float* losses, void* ws, size_t ws_bytes, int64_t n, float f0, float f1, float f2,
                       int reg_l2, int use_mask, nef_stream_t stream);
int nef_loss_noise_bwd(const float* pred, const float* pred_p, const float* pred_l, const float* target,
                       const float* noise, const float* gscale /* device scalar */, float* g_pred, float* g_p, float* g_l,
                       int64_t n, float f0, float f1, float f2, int reg_l2, int use_mask, nef_stream_t stream);

/* The structural-similarity term of the training loss (cfg.SOLVER.ssim_factor; no counterpart in the reference): factor * (1 - mean SSIM)
 * beside the three terms above, with the SSIM of nef_view_metrics (utils/metric.py:ssim_1d) so that 1 - term / factor is the number the
 * test phase reports on the same rows.  Row i of x = pred (+ noise: the same fp32 add as above) against target on [0, end_i), end_i =
 * clamp(rois[i, -1, 0], 0, L), or L with rois NULL.  7-tap uniform window, n = 7/6, c1 = 1e-4, c2 = 9e-4:
 *   S_p = (2 ux uy + c1)(2 vxy + c2) / ((ux^2 + uy^2 + c1)(vx + vy + c2)),  S_i = mean of S_p over the end_i - 6 full windows;
 *   a row with end_i < 7 has no window and is left out (zero gradient);  R = rows with a window;
 *   term = factor * (1 - (1/R) sum_i S_i),  0 with R = 0.
 * fwd (two launches behind nef_loss_*_fwd on the same stream): fp64 window arithmetic, one fp64 partial sum per (row, tile of
 *   NEF_LOSS_SSIM_TILE window starts) in ws, a one-block finish that adds them in a fixed order (no atomics: the same bits eagerly,
 *   under hipGraph replay and on every rank) and writes losses[4] = (float)term, then losses[0] = losses[0] + losses[4] (one fp32 add).
 *   `losses` has FIVE elements here.  g_pred and gscale are not read.
 * bwd (one launch behind nef_loss_*_bwd on the same stream): g_pred[i, t] += (float)g_t for t < end_i,
 *   g_t = -factor * gscale / (R (end_i - 6)) * sum over the windows p that hold t of dS_p/dx_t, in fp64 (per window a_p + b_p x_t + c_p y_t);
 *   positions t >= end_i and rows without a window are not touched.  R is derived from rois inside the launch: the entry keeps no
 *   state.  gscale: NULL (1) or the device word of nef_loss_bwd.  losses, ws and ws_bytes are not read.
 * args, pred, target, losses (fwd) / g_pred (bwd) NULL: NEF_E_NULL; B or L <= 0, B > 65535, a negative or NaN factor: NEF_E_SHAPE; fwd: ws_bytes below
 * nef_loss_ssim_ws_bytes(B, L): NEF_E_WORKSPACE, then ws NULL: NEF_E_NULL.  Every check sits in front of the launches.  Capturable: nothing
 * is read by the host, nothing is allocated. */
#define NEF_LOSS_SSIM_TILE 512
typedef struct nef_loss_ssim_args {
    const float* pred;      /* [B, L] */
    const float* target;    /* [B, L] */
    const float* noise;     /* NULL, or [B, L] */
    const int64_t* rois;    /* NULL (whole rows), or [B, 7, 2] */
    float* losses;          /* fwd: the 5-element loss row */
    void* ws;               /* fwd */
    size_t ws_bytes;        /* fwd */
    const float* gscale;    /* bwd: NULL, or a device scalar */
    float* g_pred;          /* bwd: [B, L], accumulated into */
    int32_t B;              /* rows, 1 .. 65535 */
    int32_t L;              /* row length */
    float factor;           /* >= 0 */
    int32_t reserved0;      /* 0 */
} nef_loss_ssim_args;
int nef_loss_ssim_fwd(const nef_loss_ssim_args* a, nef_stream_t stream);
int nef_loss_ssim_bwd(const nef_loss_ssim_args* a, nef_stream_t stream);
size_t nef_loss_ssim_ws_bytes(int B, int L);
/* sizeof(nef_loss_ssim_args) as the library was built. */
size_t nef_loss_ssim_args_bytes(void);

/* Wave-segment weights on the reconstruction term (cfg.SOLVER.seg_weights; no counterpart in the reference) and the per-segment squared
 * error of the test phase (cfg.SOLVER.seg_eval).  The segment of position t of row i -- ONE definition for the three entries below:
 *   end_i = clamp(rois[i, 6, 0], 0, L)                        (the row end of nef_loss_ssim_* and nef_view_metrics);
 *   t >= end_i: segment 6 (pad);  otherwise: #{k in 1..5 : rois[i, k, 0] <= t}, a value in 0..5 (P, PR, QRS, ST, T, TP).
 * Only the six start points rois[i, 1..6, 0] are read: the rule is total for any int64 content (negative, beyond L, non-monotonic, empty
 * segments) and equals "the k with rois[i, k, 0] <= t < rois[i, k, 1]" for contiguous rois.
 * fwd (two launches behind nef_loss_*_fwd on the same stream): with e(i, t) the element of the reconstruction term as nef_loss_fwd forms
 *   it in fp32 -- |d| (reg_l2 0) or d * d, d = (pred (+ noise)) - target --, S = sum_{i, t} (double)w[seg(i, t)] * (double)e(i, t): one
 *   fp64 partial per (row, tile of NEF_LOSS_SEG_TILE positions) in ws, a one-block finish that adds them in a fixed order (no atomics:
 *   the same bits eagerly, under hipGraph replay and on every rank), then losses[3] = (float)(S / (B L)) * f2 and
 *   losses[0] = (losses[1] + losses[2]) + losses[3], the association of nef_loss_fwd.  No renormalisation: all weights 1 is the flat
 *   mean.  losses[1], losses[2] and any element behind [3] keep their bits.  g_pred is not read.
 * bwd (one launch behind nef_loss_*_bwd, in front of nef_loss_ssim_bwd): g_pred[i, t] = w[seg(i, t)] * g_pred[i, t] in place, one fp32
 *   multiply and one writer per element.  Reads rois and g_pred only; keeps no state.
 * args, rois, pred / target / losses (fwd), g_pred (bwd) NULL: NEF_E_NULL; B or L <= 0, B > 65535 (the rows are a grid's y extent),
 * L % 4 != 0, a negative, infinite or NaN weight: NEF_E_SHAPE; fwd: ws_bytes below nef_loss_seg_ws_bytes(B, L): NEF_E_WORKSPACE, then ws
 * NULL: NEF_E_NULL; a tensor not 16-byte aligned: NEF_E_UNSUPPORTED.  Every check sits in front of the launches.  Capturable: nothing is
 * read by the host, nothing is allocated. */
#define NEF_LOSS_SEG_TILE 1024
typedef struct nef_loss_seg_args {
    const float* pred;      /* fwd: [B, L] */
    const float* target;    /* fwd: [B, L] */
    const float* noise;     /* fwd: NULL, or [B, L] */
    const int64_t* rois;    /* [B, 7, 2] */
    float* losses;          /* fwd: the loss row, elements [1], [2] written by nef_loss_*_fwd */
    float* g_pred;          /* bwd: [B, L], scaled in place */
    void* ws;               /* fwd */
    size_t ws_bytes;        /* fwd */
    int32_t B;              /* rows, 1 .. 65535 */
    int32_t L;              /* row length, a multiple of 4 */
    int32_t reg_l2;         /* fwd: 0 |d|, otherwise d * d */
    float f2;               /* fwd: the reconstruction term's factor */
    float w[7];             /* P, PR, QRS, ST, T, TP, pad: finite, >= 0 */
    int32_t reserved0;      /* 0 */
} nef_loss_seg_args;
int nef_loss_seg_fwd(const nef_loss_seg_args* a, nef_stream_t stream);
int nef_loss_seg_bwd(const nef_loss_seg_args* a, nef_stream_t stream);
size_t nef_loss_seg_ws_bytes(int B, int L);
/* sizeof(nef_loss_seg_args) as the library was built. */
size_t nef_loss_seg_args_bytes(void);
/* Per-segment squared error of the test phase, one block per (sample, view) row as nef_view_metrics: pred, gt fp32 [B][Q][L], rois
 * [B, 7, 2] (required); se fp64 [B][Q][7]: the sum of ((double)x - (double)y)^2 over the positions of segment k of sample b (the
 * definition above); cnt int32 [B][Q][7]: their number.  All seven bins are fixed-order block sums, no atomics.  A pointer NULL:
 * NEF_E_NULL; B, Q or L <= 0, B > 65535, L % 4 != 0: NEF_E_SHAPE; pred or gt not 16-byte aligned: NEF_E_UNSUPPORTED. */
int nef_view_seg_metrics(const float* pred, const float* gt, const int64_t* rois, double* se, int32_t* cnt, int B, int Q, int L,
                         nef_stream_t stream);

/* The slope (first-difference) term of the training loss (cfg.SOLVER.slope_factor; no counterpart in the reference): beside the terms
 * above it compares how prediction and target CHANGE from one sample to the next.  Row i of x = pred (+ noise: the same fp32 add as above)
 * against y = target on [0, end_i), end_i = clamp(rois[i, -1, 0], 0, L) (the row end of nef_loss_ssim_* and nef_view_metrics), or L with
 * rois NULL.  For t in [0, end_i - 1), in fp64 from the fp32 values and in this order:
 *   d(i, t) = ((double)x[t + 1] - (double)x[t]) - ((double)y[t + 1] - (double)y[t]);   e = |d| (l2 0) or d * d;
 *   S_i = mean of e over the end_i - 1 differences;  a row with end_i < 2 has no difference and is left out (zero gradient);
 *   R = rows with a difference;  term = factor * (1/R) sum_i S_i,  0 with R = 0.
 * Independent of the reconstruction term's factor, norm and segment weights.
 * fwd (two launches behind nef_loss_*_fwd -- and nef_loss_seg_fwd, nef_loss_ssim_fwd when they run -- on the same stream): one fp64
 *   partial sum per (row, tile of NEF_LOSS_SLOPE_TILE difference starts, staged with a one-element halo to the right) in ws, a one-block
 *   finish that adds them in a fixed order (no atomics: the same bits eagerly, under hipGraph replay and on every rank) and writes
 *   losses[slot] = (float)term, then losses[0] = losses[0] + losses[slot] (one fp32 add).  slot: 4 (a 5-element row), or 5 behind the SSIM
 *   term (a 6-element row); elements [1 .. slot - 1] keep their bits.  g_pred and gscale are not read.
 * bwd (one launch behind nef_loss_*_bwd, nef_loss_seg_bwd and nef_loss_ssim_bwd on the same stream): g_pred[i, t] += (float)g_t for
 *   t < end_i, g_t = factor * gscale / (R (end_i - 1)) * (s(t - 1) - s(t)) in fp64, s(t) = sign(d(i, t)) (sign(0) = 0; l2 0) or 2 d(i, t),
 *   s = 0 outside [0, end_i - 1); one fp32 add and one writer per element.  Positions t >= end_i and rows without a difference are not
 *   touched.  R is derived from rois inside the launch: the entry keeps no state.  gscale: NULL (1) or the device word of nef_loss_bwd.
 *   losses, ws, ws_bytes and slot are not read.
 * No alignment beyond 4 bytes is asked for and any L >= 1 is taken: rows whose pointers are 16-byte aligned are staged with 16-byte
 * loads, others element by element.
 * args, pred, target, losses (fwd) / g_pred (bwd) NULL: NEF_E_NULL; B or L <= 0, B > 65535 (the rows are a grid's y extent), a negative
 * or NaN factor, fwd: slot not 4 or 5: NEF_E_SHAPE; fwd: ws_bytes below nef_loss_slope_ws_bytes(B, L): NEF_E_WORKSPACE, then ws NULL:
 * NEF_E_NULL.  Every check sits in front of the launches.  Capturable: nothing is read by the host, nothing is allocated. */
#define NEF_LOSS_SLOPE_TILE 1024
typedef struct nef_loss_slope_args {
    const float* pred;      /* [B, L] */
    const float* target;    /* [B, L] */
    const float* noise;     /* NULL, or [B, L] */
    const int64_t* rois;    /* NULL (whole rows), or [B, 7, 2] */
    float* losses;          /* fwd: the loss row, slot + 1 elements */
    void* ws;               /* fwd */
    size_t ws_bytes;        /* fwd */
    const float* gscale;    /* bwd: NULL, or a device scalar */
    float* g_pred;          /* bwd: [B, L], accumulated into */
    int32_t B;              /* rows, 1 .. 65535 */
    int32_t L;              /* row length, >= 1 */
    float factor;           /* >= 0 */
    int32_t l2;             /* 0: |d|, otherwise d * d */
    int32_t slot;           /* fwd: 4, or 5 behind the SSIM term */
    int32_t reserved0;      /* 0 */
} nef_loss_slope_args;
int nef_loss_slope_fwd(const nef_loss_slope_args* a, nef_stream_t stream);
int nef_loss_slope_bwd(const nef_loss_slope_args* a, nef_stream_t stream);
size_t nef_loss_slope_ws_bytes(int B, int L);
/* sizeof(nef_loss_slope_args) as the library was built. */
size_t nef_loss_slope_args_bytes(void);
/* Squared slope error of the test phase (cfg.SOLVER.slope_eval), one block per (sample, view) row as nef_view_metrics: pred, gt fp32
 * [B][Q][L], rois NULL (whole rows) or [B, 7, 2]; se fp64 [B][Q]: the sum of d * d over the row's differences (the definition above
 * without noise); cnt int32 [B][Q]: their number, max(end_i - 1, 0).  Fixed-order block sums, no atomics.  pred, gt, se or cnt NULL:
 * NEF_E_NULL; B, Q or L <= 0, B * Q > 2^31 - 1: NEF_E_SHAPE. */
int nef_view_slope_metrics(const float* pred, const float* gt, const int64_t* rois, double* se, int32_t* cnt, int B, int Q, int L,
                           nef_stream_t stream);

/* The correlation term of the training loss (cfg.SOLVER.corr_factor; no counterpart in the reference): 1 - the Pearson correlation
 * coefficient of prediction and target, which no gain and no baseline offset of the prediction changes.  Row i of x = pred (+ noise: the
 * same fp32 add as above) against y = target on [0, n_i), n_i = clamp(rois[i, -1, 0], 0, L) (the row end of nef_loss_ssim_*,
 * nef_loss_slope_* and nef_view_metrics), or L with rois NULL.  In fp64 from the fp32 values, on values shifted by the row's first sample
 * (exact in fp64; a constant row then has moments that are exact zeros), u_t = x_t - x_0, w_t = y_t - y_0:
 *   mu = (1/n) sum u;  mw = (1/n) sum w;  vx = (1/n) sum u^2 - mu^2;  vy = (1/n) sum w^2 - mw^2;  c = (1/n) sum u w - mu mw;
 *   D = sqrt((vx + eps) (vy + eps));  r_i = (c + eps) / D   -- in (-1, 1]; exactly 1.0 for x == y and for two constant rows;
 *   a row with n_i < 2 is left out (zero gradient);  R = rows that count;  term = factor * (1/R) sum_i (1 - r_i),  0 with R = 0.
 * Independent of the reconstruction term's factor, norm and segment weights.
 * fwd (two launches behind nef_loss_*_fwd -- and nef_loss_seg_fwd, nef_loss_ssim_fwd, nef_loss_slope_fwd when they run -- on the same
 *   stream): the five sums of each (row, tile of NEF_LOSS_CORR_TILE positions) in ws, a one-block finish that walks rows and tiles in a
 *   fixed order (no atomics: the same bits eagerly, under hipGraph replay and on every rank) and writes losses[slot] = (float)term, then
 *   losses[0] = losses[0] + losses[slot] (one fp32 add).  slot: 4, 5 or 6 -- the term is the last element of its row, behind the SSIM and
 *   slope elements; elements [1 .. slot - 1] keep their bits.  g_pred and gscale are not read.
 * bwd (three launches behind nef_loss_*_bwd, nef_loss_seg_bwd, nef_loss_ssim_bwd and nef_loss_slope_bwd on the same stream; no state from
 *   the forward): the same partial sums into ws, a one-block finish that writes mu, mw, a_i = -factor / (R n_i D) and
 *   k_i = r_i D / (vx + eps) per row behind them, and an apply launch: g_pred[i, t] += (float)(gscale * a_i * ((w_t - mw) - k_i (u_t -
 *   mu))) for t < n_i; one fp32 add and one writer per element.  Positions t >= n_i and rows that do not count are not touched.  R is
 *   derived from rois inside the launch.  gscale: NULL (1) or the device word of nef_loss_bwd.  losses and slot are not read.
 * No alignment beyond 4 bytes is asked for and any L >= 1 is taken: tiles whose pointers are 16-byte aligned use 16-byte accesses, others
 * go element by element.
 * args, pred, target, losses (fwd) / g_pred (bwd) NULL: NEF_E_NULL; B or L <= 0, B > 65535 (the rows are a grid's y extent), a negative
 * or NaN factor or eps, fwd: slot outside 4 .. 6: NEF_E_SHAPE; ws_bytes below nef_loss_corr_ws_bytes(B, L): NEF_E_WORKSPACE, then ws
 * NULL: NEF_E_NULL.  Every check sits in front of the launches.  Capturable: nothing is read by the host, nothing is allocated. */
#define NEF_LOSS_CORR_TILE 1024
typedef struct nef_loss_corr_args {
    const float* pred;      /* [B, L] */
    const float* target;    /* [B, L] */
    const float* noise;     /* NULL, or [B, L] */
    const int64_t* rois;    /* NULL (whole rows), or [B, 7, 2] */
    float* losses;          /* fwd: the loss row, slot + 1 elements */
    void* ws;               /* 8-byte aligned; fwd and bwd may share one (stream order) */
    size_t ws_bytes;        /* at least nef_loss_corr_ws_bytes(B, L) */
    const float* gscale;    /* bwd: NULL, or a device scalar */
    float* g_pred;          /* bwd: [B, L], accumulated into */
    double eps;             /* >= 0 */
    int32_t B;              /* rows, 1 .. 65535 */
    int32_t L;              /* row length, >= 1 */
    float factor;           /* >= 0 */
    int32_t slot;           /* fwd: 4, 5 or 6 */
} nef_loss_corr_args;
int nef_loss_corr_fwd(const nef_loss_corr_args* a, nef_stream_t stream);
int nef_loss_corr_bwd(const nef_loss_corr_args* a, nef_stream_t stream);
size_t nef_loss_corr_ws_bytes(int B, int L);
/* sizeof(nef_loss_corr_args) as the library was built. */
size_t nef_loss_corr_args_bytes(void);
/* Moments of the test phase's correlation coefficient (cfg.SOLVER.corr_eval), one block per (sample, view) row as nef_view_metrics: pred,
 * gt fp32 [B][Q][L], rois NULL (whole rows) or [B, 7, 2]; mom fp64 [B][Q][3] = (vx, vy, c) by the definition above without noise (zeros
 * for an empty row); cnt int32 [B][Q] = n_i.  The host forms r = (c + eps) / sqrt((vx + eps) (vy + eps)) for the rows with cnt >= 2.
 * Fixed-order block sums, no atomics.  pred, gt, mom or cnt NULL: NEF_E_NULL; B, Q or L <= 0, B * Q > 2^31 - 1: NEF_E_SHAPE. */
int nef_view_corr_metrics(const float* pred, const float* gt, const int64_t* rois, double* mom, int32_t* cnt, int B, int Q, int L,
                          nef_stream_t stream);

/* Locating a lead's viewing angle by a scored panorama search (Model_nefnet.locate, engine.locate; no counterpart in the reference):
 * every (sample, candidate angle) view of a sweep is scored against the sample's observed rows, the best candidate is kept under a
 * deterministic rule, and the next level's candidates are laid around it.  Three entries, additions to ABI 22; all of them check their
 * arguments in front of any device work, read nothing on the host and allocate nothing (stream-ordered, capturable).
 *
 * Row length: n_i = clamp(rois[i, -1, 0], 0, L) (nef_row_end), or L with rois NULL.
 * Score of the fp32 view p against the fp32 observed row y on [0, n_i), formed in fp64 from the fp32 values; lower is better:
 *   mode 0 ('mse'):  (1/n) sum (p_t - y_t)^2;  +inf with n_i < 1.
 *   mode 1 ('corr'): 1 - r, r as nef_loss_corr_args defines it (sums on values shifted by each row's first sample, u = p - p_0,
 *     w = y - y_0; r = (c + eps) / sqrt((vx + eps) (vy + eps)));  +inf with n_i < 2.  No gain or offset of y changes it.
 *   A NaN score is stored as +inf.  p == y gives exactly 0 in both modes.
 * Best rule: candidates in order, a strictly lower score replaces the running best (ties go to the earliest candidate); with no finite
 *   score: index -1, theta NaN, score +inf.
 *
 * nef_locate_score: one wave per (sample, candidate) row, four rows of one sample per 256-thread block.  A row of up to
 *   NEF_LOCATE_SEG positions stays in the wave's registers while the wave walks the R observed rows (small: they hit L2), so every view is
 *   read from HBM once; a longer row is walked segment by segment per observed row.  Lane l owns the float4 groups q with q % 64 == l, in
 *   rising order, and the last partial group's elements one by one: 16-byte loads where a row's pointer is 16-byte aligned, scalar loads
 *   otherwise, the SAME order of additions on both, then a fixed butterfly over the 64 lanes -- a row's score depends on that row alone, not
 *   on A, the chunking or the alignment.  No atomics, no LDS, no scratch.
 *   group == 0: every candidate against every observed row, scores[b, r, col_off + a]; group == G > 0: A == R * G, candidate a belongs
 *   to observed row a / G, scores[b, a / G, col_off + a % G].
 *   args, pred, obs or scores NULL: NEF_E_NULL; B, A, R or L < 1, L > 2^30, B * ceil(A / 4) > 2^31 - 1, group < 0, A != R * group under grouping, a
 *   negative stride or column offset, a mode other than 0 / 1, eps not finite or <= 0: NEF_E_SHAPE.
 * nef_locate_best: one wave per (sample, observed row) applies the best rule to scores[b, r, 0 .. A) (a slice: sc_bs / sc_rs strides) and
 *   the matching candidates -- a shared table cands [A, 2] (per_pair 0) or the pair's own cands [B, R * A, 2] rows [r * A, (r + 1) * A)
 *   (per_pair 1) -- and merges into best_score [B, R] fp64, best_theta [B, R, 2] fp32, best_index [B, R] int64, in place.  init 1: the
 *   three are written from scratch (nothing is read); init 0: the running best is kept unless a candidate is strictly lower.
 *   keep_index 0: a winner's index is index_base + its column (level 0, chunk by chunk); keep_index 1 (later levels): best_index is not
 *   written, and a pair whose best_index is -1 is left as it is.
 *   NULL pointers: NEF_E_NULL; B, R or A < 1, B * R > 2^31 - 1, a negative stride or index_base: NEF_E_SHAPE.
 * nef_locate_cands: cands[b, r * G + i * (2 radius + 1) + k] = centre + ((float)(i - radius) * s1, (float)(k - radius) * s2),
 *   G = (2 radius + 1)^2, i-major, each coordinate one rounded fp32 multiply and one rounded fp32 add (no contraction), so the middle
 *   candidate is the centre itself.  centre = best_theta[b, r], or (ph1, ph2) -- a finite placeholder -- where best_index[b, r] < 0.
 *   Angles are neither wrapped nor clamped.  NULL pointers: NEF_E_NULL; B or R < 1, radius < 0 or > 16, B * R * G > 2^31 - 1, a step or
 *   placeholder that is not finite: NEF_E_SHAPE. */
#define NEF_LOCATE_SEG 1024
typedef struct nef_locate_score_args {
    const float* pred;      /* views [B, A, L]: element (b, a, t) at pred[b * pred_bs + a * pred_as + t] */
    const float* obs;       /* observed rows [B, R, L]: (b, r, t) at obs[b * obs_bs + r * obs_rs + t] */
    const int64_t* rois;    /* NULL (whole rows), or [B, 7, 2] */
    double* scores;         /* (b, r, j) at scores[b * sc_bs + r * sc_rs + col_off + j] */
    int64_t pred_bs;        /* element strides, >= 0 */
    int64_t pred_as;
    int64_t obs_bs;
    int64_t obs_rs;
    int64_t sc_bs;
    int64_t sc_rs;
    int64_t col_off;        /* first column written, >= 0 */
    double eps;             /* mode 1: > 0 and finite (checked in both modes) */
    int32_t B;              /* samples, >= 1 */
    int32_t A;              /* candidates per sample, >= 1 */
    int32_t R;              /* observed rows per sample, >= 1 */
    int32_t L;              /* row length, >= 1 */
    int32_t mode;           /* 0 'mse', 1 'corr' */
    int32_t group;          /* 0: all pairs; G > 0: A == R * G, candidate a against row a / G */
} nef_locate_score_args;
int nef_locate_score(const nef_locate_score_args* a, nef_stream_t stream);
/* sizeof(nef_locate_score_args) as the library was built. */
size_t nef_locate_score_args_bytes(void);
typedef struct nef_locate_best_args {
    const double* scores;   /* (b, r, j) at scores[b * sc_bs + r * sc_rs + j], j < A */
    const float* cands;     /* per_pair 0: [A, 2]; per_pair 1: [B, R * A, 2] */
    double* best_score;     /* [B, R] */
    float* best_theta;      /* [B, R, 2] */
    int64_t* best_index;    /* [B, R] */
    int64_t sc_bs;          /* element strides, >= 0 */
    int64_t sc_rs;
    int64_t index_base;     /* keep_index 0: a winner's index is index_base + j; >= 0 */
    int32_t B;              /* samples, >= 1 */
    int32_t R;              /* observed rows per sample, >= 1 */
    int32_t A;              /* candidates per (sample, observed row), >= 1 */
    int32_t per_pair;       /* 0 shared candidates, 1 per-pair candidates */
    int32_t init;           /* 1: initialise, 0: merge into the running best */
    int32_t keep_index;     /* 1: best_index is read only (levels >= 1) */
} nef_locate_best_args;
int nef_locate_best(const nef_locate_best_args* a, nef_stream_t stream);
/* sizeof(nef_locate_best_args) as the library was built. */
size_t nef_locate_best_args_bytes(void);
typedef struct nef_locate_cands_args {
    const float* best_theta;    /* [B, R, 2] */
    const int64_t* best_index;  /* [B, R] */
    float* cands;               /* [B, R * (2 radius + 1)^2, 2] */
    float s1;                   /* this level's steps, finite */
    float s2;
    float ph1;                  /* the placeholder centre of a pair without a finite score, finite */
    float ph2;
    int32_t B;                  /* samples, >= 1 */
    int32_t R;                  /* observed rows per sample, >= 1 */
    int32_t radius;             /* 0 .. 16 */
    int32_t reserved0;          /* 0 */
} nef_locate_cands_args;
int nef_locate_cands(const nef_locate_cands_args* a, nef_stream_t stream);
/* sizeof(nef_locate_cands_args) as the library was built. */
size_t nef_locate_cands_args_bytes(void);

/* Input-lead augmentation of the train step (cfg.DATA.aug_*; no counterpart in the reference, whose only augmentation is the host-side
 * angle jitter): y = a corrupted copy of the input leads x [B, V, L]; x is never written.  Every draw comes from the counter RNG of the
 * dropout epilogues (z = mix(seed + seed_dev[0], counter); k0 = z >> 40 and k1 = (z >> 16) & 0xFFFFFF are its two 24-bit fields):
 *   per element, counter = (dense element index of x) >> 1, so elements 2k and 2k + 1 share a word (L % 4 == 0: never across rows):
 *     r = sqrt(-2 ln((k0 + 1) / 2^24)),  n_even = r cos(2 pi k1 / 2^24),  n_odd = r sin(2 pi k1 / 2^24);
 *   per row (b, v), counter = 2^62 + 4 (b V + v) + j:
 *     j = 0: A_w = wander_amp k0 / 2^24,  f_w = wander_lo + (wander_hi - wander_lo) k1 / 2^24;
 *     j = 1: phi_w = k0 / 2^24 turns,  A_h = hum_amp k1 / 2^24;
 *     j = 2: phi_h = k0 / 2^24 turns,  u_d = k1 / 2^24;
 *     j = 3, of row (b, 0) only: the fallback lead floor(V k0 / 2^24).
 * Row (b, v) is dropped when u_d < lead_drop -- unless that drops all V rows of sample b, then the fallback lead is kept.  A dropped
 * row is 0 over its whole length.  A kept row, with end_b = clamp(rois[b, R - 1, 0], 0, L) (L when crop is 0):
 *   y = x + noise_std n_t + A_w sin(2 pi (f_w t / sample_rate + phi_w)) + A_h sin(2 pi (hum_hz t / sample_rate + phi_h))   for t < end_b,
 *   y = x (the bits)                                                                                                         for t >= end_b.
 * A term whose amplitude is 0 is not evaluated: with lead_drop alone, kept rows are bit copies.  The row parameters and the phase (in
 * turns, reduced to [0, 1)) are fp64; the transcendental functions and the three adds (left to right as written) are fp32.
 * One workgroup per (row, tile of NEF_AUGMENT_TILE positions), one 16-byte load and store per thread, one writer per element, no
 * atomics: the same bits eagerly, under hipGraph replay (seed_dev: the replayed step's seed word) and on every rank at one seed.
 * args, x, y NULL, or crop set with rois NULL: NEF_E_NULL; B, V, L <= 0, L % 4 != 0, R <= 0 with rois, more than 2^31 - 1 workgroups,
 * a negative or NaN amplitude, lead_drop outside [0, 1), sample_rate <= 0, wander_lo > wander_hi, wander_hi or hum_hz at or above
 * sample_rate / 2 while its amplitude is on: NEF_E_SHAPE; x or y not 16-byte aligned, or the two overlapping: NEF_E_UNSUPPORTED.
 * Every check sits in front of the launch.  Capturable: nothing is read by the host, nothing is allocated. */
#define NEF_AUGMENT_TILE 1024
typedef struct nef_augment_args {
    const float* x;             /* [B, V, L] */
    const int64_t* rois;        /* NULL, or [B, R, 2] */
    float* y;                   /* [B, V, L], not x */
    const uint64_t* seed_dev;   /* NULL, or a device word added to seed when the launch runs */
    uint64_t seed;
    double wander_amp, wander_lo, wander_hi;   /* signal units, Hz, Hz */
    double hum_amp, hum_hz;
    double sample_rate;         /* Hz, > 0 */
    float noise_std;            /* >= 0 */
    float lead_drop;            /* in [0, 1) */
    int32_t B, V, L;
    int32_t R;                  /* rois per sample (7) */
    int32_t crop;               /* 1: corrupt t < rois[b, R - 1, 0] only */
    int32_t reserved0;          /* 0 */
} nef_augment_args;
int nef_augment(const nef_augment_args* a, nef_stream_t stream);
/* sizeof(nef_augment_args) as the library was built. */
size_t nef_augment_args_bytes(void);

/* Lead masks (cfg.MODEL.lead_mask; no counterpart in the reference): the lead mean and the Standin picks over each sample's PRESENT
 * leads.  `mask` is uint8 [B][V] on the device, read as zero / non-zero.  For sample b: P_b = the ascending list of v with
 * mask[b][v] != 0, n_b = |P_b|.
 *   mean    per channel row and position: s = lead P_b[0]; s += lead P_b[k] for k = 1 .. n_b - 1, in that order, fp32;
 *           mean = s / (float)n_b  (nef_lead_mean's expression with n_b for V: an all-ones mask gives its bits).
 *   picks   with the step's two Standin draws (c1, c2) (the two ints, or choice_dev[0..1]): p1_b = P_b[c1 mod n_b],
 *           p2_b = P_b[c2 mod n_b] (the draws are read as unsigned).  All ones: c1, c2.
 *   D       [3B][256][T] as nef_mix_fwd builds it, one rounded multiply per element: pass 0 = q * latent,
 *           pass 1 = q * cat(z1[p1_b] | z2 mean), pass 2 = q * cat(z1 mean | z2r[p2_b]).
 *   absent leads are never read (a select, not a multiply by 0): a NaN in their rows reaches no output.
 *   n_b = 0: latent and the three D rows of the sample are +0.0, its picks are -1, its backward rows (gz1, gz2r, gq) are +0.0; no
 *           flag, nothing read by the host.
 *   backward  the adjoint of the above with nef_mix_bwd(shared = 0)'s expressions in their order and n_b for V:
 *           g_mean = gD0 + gD2 (z1 half) or gD0 + gD1 (z2 half), g_pick = gD1 or gD2;  gz[v] = q * g_mean / (float)n_b
 *           + (v == pick ? q * g_pick : 0) for present v -- masked with z1 > 0 on the z1 half when relu_z1 -- and +0.0 for absent v
 *           (every row of gz1 / gz2r is written);  gq[b][c] = sum_t (g_mean * latent + g_pick * z[pick]) in fp32, one wave per row.
 *           up != 0: gD is [3B][256][2T], read through the x2-upsampling adjoint exactly as nef_mix_bwd reads it.
 * One wave per (sample, channel) row; the mask row is decoded once per row into a wave-uniform bit set of present leads, which the
 * lead loop walks with scalar instructions: no per-element branch on v.  With every pointer 16-byte aligned a row is cut into an
 * unaligned head of up to three elements, 16-byte accesses and a tail (every tensor's row has the same offset modulo 16 bytes);
 * otherwise 4-byte accesses.  The same expressions per element on every path.  One writer per element, no atomics, no scratch, no
 * state: the same bits from run to run, eagerly and under hipGraph replay.
 * nef_lead_mask_mix_fwd: q == NULL and D == NULL together: the latent only (inference).  picks: NULL, or int32 [B][2].
 * args or a required pointer NULL, q NULL without D NULL (or the reverse): NEF_E_NULL; B < 1, V outside 1..12, T outside 1..2^24,
 * B * 256 * 3 * 2 * T >= 2^62, c1 or c2 negative: NEF_E_SHAPE; a float or int32 pointer not 4-byte aligned: NEF_E_UNSUPPORTED.  Every check
 * sits in front of the launch.  Capturable. */
#define NEF_LEAD_MASK_MAX_V 12
typedef struct nef_lead_mask_mix_fwd_args {
    const float* z1;            /* [B][128V][T] */
    const float* z2r;           /* [B][128V][T] */
    const uint8_t* mask;        /* [B][V] */
    const float* q;             /* [B][256], or NULL with D NULL */
    const int32_t* choice_dev;  /* NULL, or device {c1, c2} that overrides the two ints */
    float* latent;              /* [B][256][T] */
    float* D;                   /* [3B][256][T], or NULL with q NULL */
    int32_t* picks;             /* NULL, or [B][2] = {p1_b, p2_b} */
    int32_t B, V, T;
    int32_t c1, c2;             /* >= 0 */
    int32_t reserved0;          /* 0 */
} nef_lead_mask_mix_fwd_args;
int nef_lead_mask_mix_fwd(const nef_lead_mask_mix_fwd_args* a, nef_stream_t stream);
size_t nef_lead_mask_mix_fwd_args_bytes(void);

typedef struct nef_lead_mask_mix_bwd_args {
    const float* gD;            /* [3B][256][T], or [3B][256][2T] with up */
    const float* latent;        /* [B][256][T], the forward's */
    const float* z1;            /* [B][128V][T] */
    const float* z2r;           /* [B][128V][T] */
    const float* q;             /* [B][256] */
    const uint8_t* mask;        /* [B][V] */
    const int32_t* choice_dev;  /* as in the forward */
    float* gz1;                 /* [B][128V][T] */
    float* gz2r;                /* [B][128V][T] */
    float* gq;                  /* [B][256] */
    int32_t B, V, T;
    int32_t c1, c2;
    int32_t relu_z1;            /* != 0: gz1 also carries the mask z1 > 0 */
    int32_t up;                 /* != 0: gD is wrt the x2-upsampled D */
    int32_t reserved0;          /* 0 */
} nef_lead_mask_mix_bwd_args;
int nef_lead_mask_mix_bwd(const nef_lead_mask_mix_bwd_args* a, nef_stream_t stream);
size_t nef_lead_mask_mix_bwd_args_bytes(void);

/* mask[b][v] = 0 where nef_augment with the same (seed, seed_dev, lead_drop, B, V) zeroes row (b, v), 1 elsewhere: the row draw, the
 * "all dropped" test and the fallback lead are ONE device function shared with nef_augment (csrc/aug_drop.h).  lead_drop == 0: all
 * ones.  One thread per (b, v).  args or mask NULL: NEF_E_NULL; B < 1, V outside 1..12, B * V >= 2^31, lead_drop outside [0, 1) or
 * NaN: NEF_E_SHAPE.  Capturable. */
typedef struct nef_augment_mask_args {
    uint8_t* mask;              /* [B][V] */
    const uint64_t* seed_dev;   /* NULL, or a device word added to seed when the launch runs */
    uint64_t seed;
    float lead_drop;            /* in [0, 1) */
    int32_t B, V;
    int32_t reserved0;          /* 0 */
} nef_augment_mask_args;
int nef_augment_mask(const nef_augment_mask_args* a, nef_stream_t stream);
size_t nef_augment_mask_args_bytes(void);

/* The train step's label-noise row, made on the device (cfg.DATA.device_noise; the reference's DATA.noise row, solver.py:185-186, is a
 * host draw of its loader): out [Rw][L] is the addend the loss entries take as `noise`, a Gaussian draw per position whose sigma is the
 * standard deviation of the quiet second half of the row's T-P segment, measured on the TARGET row itself.  Rows are the step's final
 * fp32 target rows (Rw = B, or Q * B view-major) with their rois [Rw][7][2].  Per row i:
 *   end   = clamp(rois[i][6][0], 0, L)                      (the row end of the SSIM, slope and correlation terms)
 *   q0    = floor((rois[i][5][0] + rois[i][5][1]) / 2)      (the exact integer sum, true floor for a negative one)
 *   q1    = rois[i][5][1]
 *   [q0, q1) is cut to [0, end): q0' = clamp(q0, 0, end), q1' = clamp(q1, 0, end), m = max(q1' - q0', 0).  Only clamped values reach an
 *   address: `rois` may hold anything.
 *   sigma = sqrt(sum_t (v_t - mean)^2 / m),  mean = sum_t v_t / m  over t in [q0', q1'), in fp64 from the fp32 values (two passes, a
 *           fixed order that depends on the segment alone): the population standard deviation.  m == 0: sigma = 0 (the host row would
 *           be NaN).  A NaN in the segment: sigma is NaN.
 *   out[i][t] = (float)sigma * n_t  for t < end,  +0.0 for t >= end -- and +0.0 for every t when (float)sigma == 0.  n_t is the
 *           per-element stream of nef_augment_args under seed + seed_dev[0]: counter = (i L + t) >> 1, r = sqrt(-2 ln((k0 + 1) / 2^24)),
 *           n_even = r cos(2 pi k1 / 2^24), n_odd = r sin(2 pi k1 / 2^24), the same fp32 expressions; a row end that splits a pair
 *           leaves the element behind it +0.0.
 *   sigma[i] (when given) = sigma, fp64.
 * One 256-thread workgroup per row; the reduction is a function of the row's own data, not of Rw or the launch.  One writer per
 * element, no atomics, no scratch, no state: the same bits eagerly and under hipGraph replay (seed_dev: the replayed step's seed word).
 * args, target, rois or out NULL: NEF_E_NULL; Rw < 1, L <= 0, L % 4 != 0: NEF_E_SHAPE; target or out not 16-byte aligned, rois, sigma or
 * seed_dev not 8-byte aligned, target and out overlapping: NEF_E_UNSUPPORTED.  Every check sits in front of the launch.  Capturable. */
typedef struct nef_noise_row_args {
    const float* target;        /* [Rw][L] */
    const int64_t* rois;        /* [Rw][7][2] */
    float* out;                 /* [Rw][L], not target */
    double* sigma;              /* NULL, or [Rw] */
    const uint64_t* seed_dev;   /* NULL, or a device word added to seed when the launch runs */
    uint64_t seed;
    int32_t Rw, L;
} nef_noise_row_args;
int nef_noise_row(const nef_noise_row_args* a, nef_stream_t stream);
size_t nef_noise_row_args_bytes(void);

/* Time warp of a whole train batch with jittered marks (cfg.DATA.aug_warp / aug_roi_jitter; no counterpart in the reference): every
 * segment of every beat is resampled to a drawn multiple of its length -- inputs, target and rest views alike -- and the marks follow,
 * each interior one then moved by a drawn integer.  Out of place; no input is written.  Per sample i, with L the row length and
 * clamp(v, lo, hi) = min(max(v, lo), hi):
 *   1. edges    c_0 = clamp(rois[i,0,0], 0, L),  c_k = clamp(max(rois[i,k,0], c_{k-1}), 0, L) for k = 1..6,  n_k = c_{k+1} - c_k for k = 0..5.
 *               Only the clamped values enter any arithmetic or any address: `rois` may hold anything.
 *   2. draws    z_k = mix(seed, 2^62 + 8 (index0 + i) + k), k = 0..5 (uint64 wrap-around; mix is the counter RNG of the dropout epilogues);
 *               u_k = (z_k >> 40) 2^-24;  s_k = 1.0 + amp[k] * (2.0 * u_k - 1.0) in fp64.
 *   3. lengths  m_k = 0 when n_k == 0, else max(1, (int64)floor((double)n_k * s_k + 0.5)).  A cropped beat (c_6 == L: the signal goes on
 *               behind the row) is not warped, m_k = n_k: shrinking it would label live signal as padding.
 *   4. new edges d_0 = c_0, d_{k+1} = min(d_k + m_k, L): a stretched beat is cut at L.  The mapping below uses the uncut m_k.
 *   5. values, for every row x -> y of the sample (V inputs, the target, R rest views):
 *               t < d_0: y[t] = x[t] (the bits);  t >= d_6: y[t] = +0.0;  t in [d_k, d_{k+1}), j = t - d_k:
 *               r = (double)n_k / (double)m_k,  p = clamp((j + 0.5) * r - 0.5, 0, n_k - 1),  i0 = floor(p),  f = p - i0,
 *               i1 = min(i0 + 1, n_k - 1),  x0 = x[c_k + i0],  x1 = x[c_k + i1] as fp64,
 *               y[t] = (float)x0 when f == 0, else (float)(x0 + f * (x1 - x0)): fp64 without contraction, one rounding to fp32.
 *               (The half-pixel convention of the ROI resampling; a segment reads nothing from its neighbours.)
 *   6. marks    e_0 = d_0, e_6 = d_6; for k = 1..5 in order: j_k = (int)(((2 J + 1) * ((z_k >> 16) & 0xFFFFFF)) >> 24) - J with
 *               J = jitter, e_k = clamp(d_k + j_k, e_{k-1}, d_6).  rois_out[i,k] = [e_k, e_{k+1}] for k = 0..5 and
 *               rois_out[i,6] = [e_6, rois[i,6,1]].  The signal does not move with the jitter.
 * Zero amplitudes and jitter 0 return a beat whose rois are contiguous and in range and whose padding is zero bit for bit.  A sample's
 * result is a function of seed, index0 + i and its own rows.
 * One 256-thread workgroup per sample; a wave owns one row at a time, a lane four neighbouring outputs = one 16-byte store; wave 0 writes
 * rois_out.  One writer per element, no atomics, no scratch.
 * args, data, target, rois or an output NULL, rest or rest_out NULL with R > 0: NEF_E_NULL; B < 1, V outside 1..12, R outside 0..64,
 * L outside 4 .. 2^24 or L % 4 != 0, an amplitude outside [0, 0.9] (or NaN), jitter outside 0..64: NEF_E_SHAPE; a pointer not 16-byte
 * aligned, or an output that overlaps an input: NEF_E_UNSUPPORTED.  Every check sits in front of the launch.  Capturable: nothing is read
 * by the host, nothing is allocated. */
#define NEF_WARP_MAX_AMP 0.9
#define NEF_WARP_MAX_JITTER 64
typedef struct nef_warp_args {
    const float* data;          /* [B, V, L] */
    const float* target;        /* [B, L] */
    const float* rest;          /* [B, R, L]; NULL with R == 0 */
    const int64_t* rois;        /* [B, 7, 2], any content */
    float* data_out;            /* [B, V, L] */
    float* target_out;          /* [B, L] */
    float* rest_out;            /* [B, R, L]; NULL with R == 0 */
    int64_t* rois_out;          /* [B, 7, 2] */
    uint64_t seed;
    int64_t index0;             /* sample i draws as sample index0 + i */
    double amp[6];              /* P, PR, QRS, ST, T, TP: each in [0, 0.9] */
    int32_t jitter;             /* J in 0 .. 64 */
    int32_t B, V, R, L;
    int32_t reserved0;          /* 0 */
} nef_warp_args;
int nef_warp(const nef_warp_args* a, nef_stream_t stream);
/* sizeof(nef_warp_args) as the library was built. */
size_t nef_warp_args_bytes(void);

/* Tianchi train / test batches built on the device from recordings kept in device memory (cfg.DATA.device_resident; the host path is
 * dataset/tianchi.py, EcgTianChiInterval.__getitem__, whose bits this entry promises).  `signal` holds every recording's eight stored
 * leads, lead-major per recording ([8, len_i], recordings concatenated), as int16 (dtype 0) or fp32 (dtype 1) elements.  `plan` is the
 * host's draw for the batch, one row of W = 3 + V + 1 + R int64 words per sample:
 *   [0] element index of lead 0 at the beat's P onset   [1] the recording's lead stride (its length)   [2] n = end - p_on
 *   [3 .. 3 + V) the input leads   [3 + V] the target lead   [4 + V .. W) the rest leads          (lead indices 0..11; 8..11 are derived)
 * With I, II the stored leads 0 and 1, the derived leads are 8: II - I, 9: -0.5 * (I + II), 10: I - 0.5 * II, 11: II - 0.5 * I, formed in
 * fp64 without contraction.  Per sample: lo / hi = min / max over all 12 leads and all n positions (NaN propagates, as numpy.min does); output
 * row r (r-th lead of the plan row) holds (float)((s - lo) / (hi - lo)) at t < n, in fp64 with IEEE division and one rounding, and 0.0f at
 * n <= t < 512.  hi == lo gives what IEEE gives (NaN).  n may exceed 512: lo / hi see the whole beat, the rows its first 512 positions.
 * One workgroup per sample, no atomics, one writer per element, 16-byte stores; a row is read with 16- / 8- / 4-byte loads where its first
 * element's address allows and element by element otherwise, the values are the same either way.
 * A plan row that points outside `signal` (offset < 0, n < 1, n > stride, offset + 7 * stride + n > signal_elems) or names a lead outside
 * 0..11 reads nothing: all of that sample's output rows are NaN.
 * B < 1, V outside 1..12, R outside 0..64, dtype outside {0, 1}, signal_elems < 1: NEF_E_SHAPE; a NULL pointer (rest_view may be NULL
 * only with R == 0): NEF_E_NULL; signal, data, target_view or rest_view not 16-byte aligned: NEF_E_UNSUPPORTED.  Every check sits in front
 * of the launch.  Capturable: nothing is read by the host, nothing is allocated. */
#define NEF_BEAT_LEN 512
typedef struct nef_beat_batch_args {
    const void* signal;         /* int16 or fp32 elements */
    const int64_t* plan;        /* [B, 3 + V + 1 + R] */
    float* data;                /* [B, V, 512] */
    float* target_view;         /* [B, 512] */
    float* rest_view;           /* [B, R, 512]; NULL with R == 0 */
    int64_t signal_elems;       /* elements in `signal` */
    int32_t B;
    int32_t V;
    int32_t R;
    int32_t dtype;              /* 0: int16, 1: fp32 */
} nef_beat_batch_args;
int nef_beat_batch(const nef_beat_batch_args* a, nef_stream_t stream);
/* sizeof(nef_beat_batch_args) as the library was built. */
size_t nef_beat_batch_args_bytes(void);

/* Whole recordings from per-beat views (recording.py): the three entries that take nef_beat_batch's direction back.  All are
 * capturable and stateless, use no atomics and no scratch, and give every output element one writer.  `views` and `out` may sit at any
 * 4-byte address: a row whose first element is 16-byte aligned moves in 16-byte accesses, another one element by element, the values
 * being the same either way.
 *
 * nef_beat_range: range[b] = (lo, hi) of plan row b, formed exactly as nef_beat_batch forms them (all 12 leads, all n positions, fp64, a
 * NaN wins) from the same `signal` and the same plan of W = 3 + V + 1 + R words per row.  One workgroup per row.  A row that leaves `signal`
 * or names a lead outside 0..11 -- the rows nef_beat_batch answers with NaNs -- reads nothing and gives (NaN, NaN).
 * B < 1, V outside 1..12, R outside 0..64, dtype outside {0, 1}, signal_elems < 1: NEF_E_SHAPE; a NULL pointer: NEF_E_NULL; signal not
 * 16-byte aligned, plan or range not 8-byte aligned: NEF_E_UNSUPPORTED. */
typedef struct nef_beat_range_args {
    const void* signal;         /* int16 or fp32 elements */
    const int64_t* plan;        /* [B, 3 + V + 1 + R] */
    double* range;              /* [B, 2]: lo, hi */
    int64_t signal_elems;
    int32_t B;
    int32_t V;
    int32_t R;
    int32_t dtype;              /* 0: int16, 1: fp32 */
} nef_beat_range_args;
int nef_beat_range(const nef_beat_range_args* a, nef_stream_t stream);
size_t nef_beat_range_args_bytes(void);

/* nef_beat_stitch: views[b, a, 0..512) (fp32; beat b's angle row a starts at views + b * view_bs + a * view_as, strides in elements, the
 * row itself contiguous) is beat b of a recording seen from angle a in the beat's own normalisation.  With (lo, hi) = range[b],
 * span = hi - lo, and table row b =
 *   [0] element index in `out` of angle 0 at the beat's P onset   [1] the recording's length = the angle stride of its [A, len] signals
 *   [2] n = end - p_on                                             [3] 1: row b + 1 is the following beat of the same recording, else 0
 * it writes, for every a < A,
 *   t < min(n, 512):  out[[0] + a * [1] + t] = (float)(lo + (double)views[b, a, t] * span)      one fp64 multiply, one fp64 add, one rounding
 *   512 <= t < n:     fill 0: NaN.  fill 1 ("bridge"): (float)(a0 + (a1 - a0) * ((double)(t - 511) / (double)(n - 511))), a0 this beat's
 *                     fp64 value at t = 511 and a1 the next row's fp64 value at t = 0 where [3] == 1 (and b + 1 < Bt), else a0 (hold).
 * hi == lo gives the constant lo.  A range whose span is not finite makes every value formed with it NaN.  Positions outside every beat
 * are never written.  A table row that would leave `out` (offset < 0, n < 1, n > stride, [0] + (A - 1) * [1] + n > out_elems) writes
 * nothing; the check is inside the launch, per block.  Grid (groups of 4 angles, beat): a wave per angle row, 8 positions per lane, the
 * tail beyond 512 strided over the wave.
 * Bt outside 1..65535, A outside 1..65536, fill outside {0, 1}, out_elems outside [1, 2^40), view_as < 512, view_bs < A * view_as:
 * NEF_E_SHAPE; a NULL pointer: NEF_E_NULL; views or out not 4-byte aligned, range or table not 8-byte aligned: NEF_E_UNSUPPORTED. */
typedef struct nef_beat_stitch_args {
    const float* views;         /* [Bt, A, 512] through view_bs / view_as */
    const double* range;        /* [Bt, 2] */
    const int64_t* table;       /* [Bt, 4] */
    float* out;                 /* out_elems floats */
    int64_t view_bs;            /* elements between beats */
    int64_t view_as;            /* elements between the angle rows of a beat */
    int64_t out_elems;
    int32_t Bt;
    int32_t A;
    int32_t fill;               /* 0: NaN, 1: bridge */
    int32_t reserved0;          /* 0 */
} nef_beat_stitch_args;
int nef_beat_stitch(const nef_beat_stitch_args* a, nef_stream_t stream);
size_t nef_beat_stitch_args_bytes(void);

/* nef_recording_stats: stats[i, a, 0..7) of the stitched signal x = out[out_offsets[i] + a * len_i + .] against the truth y = lead
 * score_leads[a] (0..11; 8..11 derived as nef_beat_batch derives them; -1: none, seven zeros) of recording i, whose eight stored leads sit
 * at signal[[2] .. [2] + 8 * [3]) of rec_table row i = [first row of beat_table, number of rows, offset in `signal`, len_i].  beat_table is
 * nef_beat_stitch's table.  Covered positions: the first min(n, 512) of each of the recording's beats, all n with fill 1.  In fp64 from
 * the fp32 / stored values, with u = x - x_first and w = y - y_first shifted by the recording's first covered sample and d = x - y:
 *   [0] count   [1] sum d^2   [2] sum u   [3] sum w   [4] sum u^2   [5] sum w^2   [6] sum u w
 * A NaN in x propagates into the sums.  One workgroup per (recording, angle); wave w takes the recording's beats w, w + 4, ..., lane l the
 * groups of 8 positions l, l + 64, ... of a beat; lanes are summed by a shuffle tree and the four waves in order, so a result depends on
 * the recording's own rows alone -- not on N, A or the rest of the launch.  A recording that would leave `signal` or `out`, a beat outside
 * its recording or a lead outside -1..11 reads nothing and gives seven NaNs.
 * Bt, N or A < 1, A > 65536, N * A >= 2^31, fill or dtype outside {0, 1}, out_elems outside [1, 2^40), signal_elems < 1: NEF_E_SHAPE; a
 * NULL pointer: NEF_E_NULL; signal not 16-byte aligned, out or score_leads not 4-byte, a table or stats not 8-byte aligned:
 * NEF_E_UNSUPPORTED. */
typedef struct nef_recording_stats_args {
    const float* out;           /* the stitched signals */
    const void* signal;         /* int16 or fp32 elements */
    const int64_t* beat_table;  /* [Bt, 4] */
    const int64_t* rec_table;   /* [N, 4] */
    const int64_t* out_offsets; /* [N]: element index in `out` of recording i's [A, len_i] signals */
    const int32_t* score_leads; /* [A] */
    double* stats;              /* [N, A, 7] */
    int64_t out_elems;
    int64_t signal_elems;
    int32_t Bt;
    int32_t N;
    int32_t A;
    int32_t fill;               /* 0: the first 512 positions of a beat are covered, 1: all n */
    int32_t dtype;              /* 0: int16, 1: fp32 */
    int32_t reserved0;          /* 0 */
} nef_recording_stats_args;
int nef_recording_stats(const nef_recording_stats_args* a, nef_stream_t stream);
size_t nef_recording_stats_args_bytes(void);

/* Marks for unannotated recordings (dataset/marks.py): the QRS detector over a device-resident store.  Both entries are
 * capturable and stateless, use no atomics and no scratch, and give every output element one writer.  They share one device table of int64
 * rows [0] offset of the recording in `signal` (its eight stored leads as [8, len], lead-major)  [1] len  [2] offset of its envelope in `env`.
 *
 * nef_mark_envelope: with x_c the stored lead c as fp64 and the leads c of lead_bits (bit c set) in ascending order,
 *   d_c(t) = x_c[min(t + D, len - 1)] - x_c[max(t - D, 0)]        e(t) = sum_c d_c(t) * d_c(t)
 *   env[[2] + t] = sum of e(u), u from max(t - H, 0) to min(t + H, len - 1) in ascending order,
 * the multiply and each add rounded separately (fp64, no contraction).  On an int16 store every intermediate is an integer below 2^41 and the
 * order does not matter; on an fp32 store the order above is the definition.  One workgroup per (recording, tile of NEF_MARK_TILE
 * positions), the tile of e and its H halo staged in LDS once; any offset alignment and any len >= 1 give the same values.  A row that would
 * leave `signal` or `env`, or whose len is below 1 or above max_len (the grid covers max_len positions), writes nothing; the check is inside
 * the launch, per block.
 * N outside 1..65535, max_len outside 1..2^31 - 65536, D outside 0..NEF_MARK_MAX_D, H outside 0..NEF_MARK_MAX_H, lead_bits outside 1..255,
 * dtype outside {0, 1}, signal_elems or env_elems < 1: NEF_E_SHAPE; a NULL pointer: NEF_E_NULL; signal not 16-byte aligned, table or env not
 * 8-byte aligned: NEF_E_UNSUPPORTED. */
#define NEF_MARK_TILE 1024
#define NEF_MARK_MAX_D 4096
#define NEF_MARK_MAX_H 256
#define NEF_MARK_MAX_R 512
#define NEF_MARK_MAX_SEGMENTS 4096
typedef struct nef_mark_envelope_args {
    const void* signal;         /* int16 or fp32 elements */
    const int64_t* table;       /* [N, 3] */
    double* env;                /* env_elems doubles */
    int64_t signal_elems;
    int64_t env_elems;
    int64_t max_len;            /* no row is longer */
    int32_t N;
    int32_t D;
    int32_t H;
    int32_t lead_bits;
    int32_t dtype;              /* 0: int16, 1: fp32 */
    int32_t reserved0;          /* 0 */
} nef_mark_envelope_args;
int nef_mark_envelope(const nef_mark_envelope_args* a, nef_stream_t stream);
size_t nef_mark_envelope_args_bytes(void);

/* nef_mark_peaks: the peaks of every row's envelope env[[2] .. [2] + len), one workgroup per row ([0] is not read).
 *   level   nseg = max(len / seg, 1) segments [i seg, (i + 1) seg), the last one extended to len; level = the lower median of their maxima,
 *           the element of rank (nseg - 1) / 2 in ascending order.
 *   peak    t is one iff env[t] > 0, env[t] >= level * frac (one fp64 multiply), env[u] < env[t] for every u in [max(t - r, 0), t) and
 *           env[u] <= env[t] for every u in (t, min(t + r, len - 1)]: non-maximum suppression, a plateau going to its earliest position.
 * peaks[i, 0 .. max_peaks) holds row i's peaks in ascending order, -1 behind them; count[i] is their true number, also above max_peaks;
 * level[i] the level.  A row whose envelope holds a non-finite value, that would leave `env`, or whose len is below 1 or above max_len gets
 * count -1, a NaN level and a row of -1.  No sequential state: a row's result is a function of its envelope alone.
 * N < 1, max_len outside 1..2^31 - 65536, seg < 1, max_len / seg > NEF_MARK_MAX_SEGMENTS, r outside 0..NEF_MARK_MAX_R, max_peaks outside
 * 1..2^20, frac negative, infinite or NaN, env_elems < 1: NEF_E_SHAPE; a NULL pointer: NEF_E_NULL; env, table or level not 8-byte aligned,
 * peaks or count not 4-byte aligned: NEF_E_UNSUPPORTED. */
typedef struct nef_mark_peaks_args {
    const double* env;          /* env_elems doubles */
    const int64_t* table;       /* [N, 3] */
    int32_t* peaks;             /* [N, max_peaks] */
    int32_t* count;             /* [N] */
    double* level;              /* [N] */
    int64_t env_elems;
    int64_t max_len;            /* no row is longer */
    double frac;
    int32_t N;
    int32_t seg;
    int32_t r;
    int32_t max_peaks;
} nef_mark_peaks_args;
int nef_mark_peaks(const nef_mark_peaks_args* a, nef_stream_t stream);
size_t nef_mark_peaks_args_bytes(void);

/* Resampling in time by a rational factor (resample.py; dataset/resident.py: DATA.source_rate): a polyphase FIR that
 * takes recordings stored at another rate to the model's, and synthesised strips back.  Capturable and stateless, no atomics, no scratch,
 * one writer per element; a row's output is a function of that row alone.
 *
 * Rates are positive integers in Hz: g = gcd(src, dst), up = dst / g, down = src / g; a row of len samples gives
 * out_len = (len * up + down - 1) / down.  The filter is designed on the host in fp64 (resample.design(up, down, zeros, beta)):
 *   m = max(up, down), c = zeros * m, N = 2 c + 1, h[n] = sinc((n - c) / m) * kaiser(N, beta)[n]
 *   for phase p in [0, up): first[p] = ceil((p - c) / up), cnt[p] = floor((p + c) / up) - first[p] + 1, K = max cnt
 *   raw[p, k] = h[p + c - (first[p] + k) * up] for k < cnt[p], else 0.0;  taps[p, k] = raw[p, k] / (the sum of raw[p, :] in ascending k)
 * -- normalised per phase, so that a constant row comes out as that constant.  The device receives `taps` (fp64 [up, K]) and `first`
 * (int32 [up]) and forms, for output m of a row x with i0 = (m * down) / up and p = (m * down) % up,
 *   y[m] = (float) sum_{k = 0 .. K-1} taps[p, k] * (double) x[clamp(i0 + first[p] + k, 0, len - 1)]
 * in ascending k from +0.0, every multiply and every add rounded on its own (fp64, no contraction).  The ends are edge replication; a
 * zero-padded tap still multiplies its clamped sample, so a NaN spreads exactly as the formula says.  The result is defined bit for bit
 * by the table the caller hands in.
 *
 * `table` holds N int64 rows [0] offset in `src` of `rows` lead-major signals [rows, len]  [1] len  [2] offset in `dst` of their
 * [rows, out_len] fp32 results  [3] rows.  One 256-thread workgroup per (table row, signal, tile of NEF_RESAMPLE_TILE outputs): the input
 * stretch of the tile is staged in LDS once, clamped, at any offset alignment and any len >= 1; the taps come from LDS when
 * up * K <= NEF_RESAMPLE_LDS_TAPS and from global memory otherwise, in the same order.  A row that would leave `src` or `dst`, whose len is
 * below 1, whose rows are outside 1..max_rows or whose out_len is above max_out_len (the grid covers max_rows x max_out_len) writes
 * nothing; the check is inside the launch, per block.  `first` is not trusted either: any content gives the formula's sum.
 * N or max_rows outside 1..65535, max_out_len outside 1..2^31 - 65536, up outside 1..NEF_RESAMPLE_MAX_UP, K outside 1..NEF_RESAMPLE_MAX_K,
 * down outside 1..NEF_RESAMPLE_MAX_RATIO * up, dtype outside {0, 1}, src_elems or dst_elems < 1: NEF_E_SHAPE; a NULL pointer: NEF_E_NULL;
 * src not 16-byte aligned, table or taps not 8-byte, dst or first not 4-byte aligned: NEF_E_UNSUPPORTED. */
#define NEF_RESAMPLE_TILE 1024
#define NEF_RESAMPLE_MAX_UP 1024
#define NEF_RESAMPLE_MAX_K 512
#define NEF_RESAMPLE_MAX_RATIO 8
#define NEF_RESAMPLE_LDS_TAPS 4096
typedef struct nef_resample_args {
    const void* src;            /* int16 or fp32 elements */
    const int64_t* table;       /* [N, 4] */
    float* dst;                 /* dst_elems floats */
    const double* taps;         /* [up, K] */
    const int32_t* first;       /* [up] */
    int64_t src_elems;
    int64_t dst_elems;
    int64_t max_out_len;        /* no row's out_len is larger */
    int32_t N;
    int32_t max_rows;           /* no table row holds more signals */
    int32_t up;
    int32_t down;
    int32_t K;
    int32_t dtype;              /* 0: int16, 1: fp32 */
} nef_resample_args;
int nef_resample(const nef_resample_args* a, nef_stream_t stream);
size_t nef_resample_args_bytes(void);

/* Sliding median over rows of a resident store (clean.py; dataset/resident.py: DATA.baseline_ms): the baseline estimate
 * of a recording, or the recording minus it.  Capturable and stateless, no atomics, no scratch, one writer per element; a signal's result
 * is a function of that signal alone.
 *
 * `table` holds N int64 rows [0] offset  [1] len  [2] rows: `rows` lead-major signals [rows, len] at the same offset in `src`, `dst` and
 * `minuend`.  For every signal x and every t in [0, len) the window is the 2 h + 1 values x[clamp(t + j, 0, len - 1)], j = -h .. h (edge
 * replication), taken as fp32.  m(t) is the (h + 1)-th smallest of them, ordered by value: -0.0 and +0.0 compare equal and either may come
 * out, infinities order as usual, and m(t) is NaN if any value of the window is NaN (numpy.median's rule; the window is odd, so m(t) is one
 * of its elements and nothing is averaged).
 *   minuend NULL:   dst[t] = m(t)
 *   else:           dst[t] = (float) ((double) minuend[t] - (double) m(t))          -- one rounding
 * `dst` may be an fp32 `minuend` itself: each element is read and written by the one thread that owns it.  `dst` must not overlap `src`.
 * h = 0 copies (or subtracts a value from itself).  Positions outside every row are never written.
 *
 * One 256-thread workgroup per (table row, signal, tile of NEF_MEDIAN_TILE outputs): the tile and h positions of halo on each side are
 * staged in LDS once as order-preserving 32-bit keys (u ^ (sign ? ~0 : 0x80000000), -0.0 folded onto +0.0, a NaN counted) with their
 * positions, sorted by key, and every output walks the sorted positions counting those inside its window up to h + 1; any offset alignment
 * and any len >= 1.  A row that would leave `src`, `dst` or `minuend`, whose len is outside 1..max_len or whose rows are outside
 * 1..max_rows (the grid covers max_rows x max_len) writes nothing; the check is inside the launch, per block.
 * N or max_rows outside 1..65535, max_len outside 1..2^31 - 65536, h outside 0..NEF_MEDIAN_MAX_H, dtype or minuend_dtype outside {0, 1},
 * an element count < 1: NEF_E_SHAPE; src, table or dst NULL: NEF_E_NULL; src not 16-byte aligned, table not 8-byte, dst not 4-byte,
 * minuend not aligned to its element: NEF_E_UNSUPPORTED. */
#define NEF_MEDIAN_TILE 1024
#define NEF_MEDIAN_MAX_H 512
typedef struct nef_sliding_median_args {
    const void* src;            /* int16 or fp32 elements */
    const int64_t* table;       /* [N, 3] */
    float* dst;                 /* dst_elems floats */
    const void* minuend;        /* NULL, or int16 / fp32 elements */
    int64_t src_elems;
    int64_t dst_elems;
    int64_t minuend_elems;      /* read with a minuend only */
    int64_t max_len;            /* no row is longer */
    int32_t N;
    int32_t max_rows;           /* no table row holds more signals */
    int32_t h;
    int32_t dtype;              /* of src: 0 int16, 1 fp32 */
    int32_t minuend_dtype;      /* 0 int16, 1 fp32 */
    int32_t reserved0;          /* 0 */
} nef_sliding_median_args;
int nef_sliding_median(const nef_sliding_median_args* a, nef_stream_t stream);
size_t nef_sliding_median_args_bytes(void);

/* ---------------------------------------------------------------------------------------------
 * SGD with momentum over a flat buffer.  codes/solver/optim_scheduler.py:10 (torch.optim.SGD semantics:
 * first step buf = g, afterwards buf = mu*buf + g; p -= lr*buf).  g is multiplied by gscale first
 * (1/world_size after an all-reduce sum). */
int nef_sgd_momentum(float* p, const float* g, float* buf, int64_t n, float lr, float mu, float gscale,
                     int first_step, const float* skip_if_positive /* NULL, or a device word: > 0 = leave p and buf as they are
                     (a step whose gradients are tainted, see nef_h2_taint) */, int32_t* skipped /* NULL, or a device counter of
                     skipped steps */, const float* lr_dev /* NULL, or a device word that replaces `lr` at run time (hipGraph replay: a scheduler's
                     new learning rate without a re-capture) */, nef_stream_t stream);
/* Adam over a flat buffer.  codes/solver/optim_scheduler.py:8 (torch.optim.Adam semantics with amsgrad=False, maximize=False and L2
 * weight_decay folded into the gradient): g' = g*gscale + weight_decay*p; m = lerp(m, g', 1-beta1); v = beta2*v + (1-beta2)*g'^2;
 * with t = *step + 1 and the bias corrections bc1 = 1-beta1^t, bc2 = 1-beta2^t in fp64: p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps).
 * `step` is a device word (torch's state["step"]: completed updates) that a second, one-lane launch advances behind the update, so
 * a captured launch steps the right t on every replay.  skip_if_positive / skipped / lr_dev: as for nef_sgd_momentum; a skipped step
 * leaves p, m, v and *step as they are.  16-byte aligned p, g, m, v take the vector path.  The betas are doubles because torch forms
 * 1 - beta and the bias corrections from Python floats: 1 - (double)0.999f is 1.3e-5 away from 1 - 0.999. */
int nef_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2, float eps,
             float weight_decay, float gscale, float* step /* device word: completed updates */, const float* skip_if_positive,
             int32_t* skipped, const float* lr_dev, nef_stream_t stream);
/* The update with weight decay: SGD with L2 decay and Nesterov momentum, Adam with L2 decay, AdamW, over a flat buffer in ONE launch
 * (rules 1 and 2: plus the one-lane launch that advances *step), with a decay multiplier per RUN of elements -- so that biases and
 * BatchNorm affine parameters can be exempt without a second parameter group, a mask buffer or a second launch (no counterpart in the
 * reference, which never decays).  Element i of run r is decayed with wd_i = weight_decay * run_mul[r]; torch's operation order:
 *   rule 0, torch.optim.SGD (dampening 0): g' = g*gscale + wd_i*p; buf = mu*buf + g'; d = nesterov ? g' + mu*buf : buf; p -= lr*d.
 *           buf starts at zero (torch's first step "buf = g'" in both forms; dampening != 0 would need a device step word).
 *   rule 1, torch.optim.Adam: the arithmetic of nef_adam with wd_i in place of weight_decay.
 *   rule 2, torch.optim.AdamW: p *= (float)(1.0 - (double)lr * (double)wd_i), the factor formed in fp64 like the bias corrections
 *           (lr: *lr_dev when given), then rule 1's update on the UNDECAYED gradient g*gscale.
 * A positive skip word leaves p, every state buffer and *step as they are -- the decay included -- and counts the step; lr_dev
 * replaces lr: both as for nef_sgd_momentum.  16-byte aligned p, g and state buffers take the vector path, anything else (and the
 * n % 4 tail) the scalar one.  With weight_decay = 0, nesterov = 0 and no table the results are those of nef_sgd_momentum
 * (first_step = 0) / nef_adam bit for bit; so are those of an all-zero table with weight_decay > 0.
 * THE RUN TABLE IS THE CALLER'S DUTY: this entry cannot read device memory, so nothing checks that run_end is ascending, that its
 * last element equals n or that run_mul is non-negative.  (A table that breaks this decays elements with another run's multiplier;
 * the lookup itself never leaves the n_runs entries.)  Capturable: nothing is read by the host, nothing is allocated. */
#define NEF_UPDATE_MAX_RUNS 256 /* runs of one launch (the table is staged in LDS); the model's 53 parameter tensors merge into fewer */
typedef struct nef_update_args {
    float* p;                      /* [n] parameters, updated in place */
    const float* g;                /* [n] gradients (the un-averaged sum: multiplied by gscale first) */
    float* buf;                    /* rule 0: [n] momentum buffer.  Rules 1, 2: unused */
    float* m;                      /* rules 1, 2: [n] exp_avg */
    float* v;                      /* rules 1, 2: [n] exp_avg_sq */
    float* step;                   /* rules 1, 2: device word, completed updates (nef_adam's) */
    const float* skip_if_positive; /* NULL, or a device word: > 0 = touch nothing */
    int32_t* skipped;              /* NULL, or a device counter of skipped steps */
    const float* lr_dev;           /* NULL, or a device word that replaces lr at run time */
    const int64_t* run_end;        /* NULL (n_runs = 0: multiplier 1 everywhere), or [n_runs] device int64: the exclusive end of each run in
                                      flat order, ascending, the last one = n */
    const float* run_mul;          /* NULL, or [n_runs] device floats >= 0 */
    int64_t n;
    double beta1, beta2;           /* rules 1, 2 (doubles: see nef_adam) */
    float lr, gscale;
    float mu;                      /* rule 0: momentum */
    float eps;                     /* rules 1, 2 */
    float weight_decay;            /* >= 0 */
    int32_t rule;                  /* 0 SGD, 1 Adam (L2 decay), 2 AdamW (decoupled decay); anything else: NEF_E_UNSUPPORTED */
    int32_t nesterov;              /* rule 0 */
    int32_t n_runs;                /* 0 .. NEF_UPDATE_MAX_RUNS; more: NEF_E_SHAPE */
} nef_update_args;

int nef_update(const nef_update_args* a, nef_stream_t stream);
/* sizeof(nef_update_args) as the library was built: a binding checks its mirror of the struct against it. */
size_t nef_update_args_bytes(void);
/* nef_update with one more in/out stream: an exponential moving average (EMA) of the parameters, kept inside the same launch (no
 * counterpart in the reference).  After the update of element i -- its new p still in registers -- ema[i] = fmaf(w, p[i] - ema[i],
 * ema[i]) in fp32, with w = (float)(1.0 - d_t) formed in fp64; d_t = decay, or with warmup min(decay, (1 + t) / (10 + t)) where
 * t = *n_averaged, the number of completed EMA updates (a device word like *step: every block reads it before anything changes it).
 * The one-lane launch behind the update advances *n_averaged -- for rules 1 and 2 it is the launch that advances *step, still one.
 * p, the state buffers and *step get the bits nef_update gives them for the same nef_update_args.  A positive skip word leaves ema
 * and *n_averaged as they are too; lr_dev and skipped: as for nef_update.  The vector path needs ema 16-byte aligned as well.
 * Returns what nef_update returns for `a`; e, e->ema or e->n_averaged NULL: NEF_E_NULL; decay outside [0, 1) or NaN: NEF_E_SHAPE.
 * Capturable: nothing is read by the host, nothing is allocated. */
typedef struct nef_ema_args {
    float* ema;                    /* [n] the averaged parameters, updated in place */
    float* n_averaged;             /* device word: completed EMA updates */
    double decay;                  /* in [0, 1) */
    int32_t warmup;                /* != 0: d_t = min(decay, (1 + t) / (10 + t)) */
    int32_t reserved0;             /* 0 */
} nef_ema_args;

int nef_update_ema(const nef_update_args* a, const nef_ema_args* e, nef_stream_t stream);
/* sizeof(nef_ema_args) as the library was built. */
size_t nef_ema_args_bytes(void);
/* Layer-wise trust ratios: LARS (a->rule 0, the SGD family) and LAMB (a->rule 1, the Adam family) over the flat buffers of
 * nef_update_args, with one norm pair per SEGMENT (parameter tensor) -- no counterpart in the reference or in torch.optim, so the
 * semantics are written out here.  Segment s is [beg_s, end_s) in flat order (beg_0 = 0, beg_s = seg_end[s - 1]) and carries
 * seg_wd_mul[s] >= 0 and seg_adapt[s] (0 = exempt from the ratio, anything else = adapted).  g' = g * gscale (behind the clipping when
 * nef_grad_clip ran in front), wd_s = weight_decay * seg_wd_mul[s]; norms are 2-norms over the segment, fp64 sums of the squares of
 * the fp32 values, in a fixed order (no atomics): the same buffers give the same bits eagerly, under hipGraph replay and on every rank.
 *   rule 0, LARS (momentum SGD, dampening 0, optional Nesterov): wn = ||p_s||, gn = ||g'_s||;
 *           q_s = trust_coef * wn / (gn + wd_s * wn + trust_eps) when seg_adapt[s], wn > 0 and gn > 0, else 1 -- formed in fp64, rounded
 *           to fp32 once; d = (g' + wd_s * p) * q_s; buf = mu * buf + d; p -= lr * (nesterov ? d + mu * buf : buf).  With every q_s = 1
 *           these are rule 0's bits of nef_update under a run table with the same multipliers.
 *   rule 1, LAMB: m = lerp(m, g', 1 - beta1); v = beta2 * v + (1 - beta2) * g'^2; t = *step + 1, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t
 *           in fp64 as in nef_adam; u = (m / bc1) / (sqrt(v / bc2) + eps) + wd_s * p; wn = ||p_s||, un = ||u_s||; q_s = wn / un when
 *           seg_adapt[s], wn > 0 and un > 0, else 1; p -= lr * q_s * u; *step advances.
 * Three stream-ordered launches and a one-lane one (rule 1, or with the average): a read-only norm pass (rule 1: it forms the new m,
 * v and u in registers and stores none of them; the update recomputes them from the old state in the same operation order, so the
 * u applied is the u measured), a one-block finish (ratio, stats, taint) and the update.
 *   ratio[s] = q_s of this call;  stats[0] / stats[1] = the smallest / largest q_s over the adapted segments (1 when none adapts);
 *   stats[2] += 1 per call that updated;  stats[3] += 1 per call whose norms were not finite.
 * Norms that are not finite (in any segment) skip the step: stats[3] and, if given, taint[0] advance by 1, ratio[] and stats[0..2]
 * stay as they were, and p, every state buffer, *step, the average and its count keep their bits; `skipped` counts the step once.
 * A positive skip word -- or a positive taint[0] -- on entry does the same without touching ratio, stats or taint.  lr_dev replaces lr.
 * e: NULL, or the moving average of nef_update_ema, kept inside the update launch; p and the state get the same bits with and without.
 * a->run_end / run_mul are not read: a->n_runs must be 0 (NEF_E_SHAPE), the multipliers travel per segment.  a->rule > 1:
 * NEF_E_UNSUPPORTED.  t, seg_end, seg_wd_mul, seg_adapt, ratio, stats or ws NULL: NEF_E_NULL; n_segs outside 1 .. NEF_TRUST_MAX_SEGS,
 * a negative (or NaN) trust_coef / trust_eps / weight_decay: NEF_E_SHAPE; ws_bytes below nef_update_trust_ws_bytes: NEF_E_WORKSPACE.
 * Every check sits in front of the first launch.
 * THE SEGMENT TABLE IS THE CALLER'S DUTY, as the run table of nef_update is: this entry cannot read device memory, so nothing checks
 * that seg_end is ascending, that its last element equals n or that seg_wd_mul is non-negative.  (Elements behind the last end belong
 * to no norm and are updated with the last segment's factors; the lookups never leave the n_segs entries.)
 * Capturable: nothing is read by the host, nothing is allocated. */
#define NEF_TRUST_MAX_SEGS 256 /* segments of one call (the table is staged in LDS; the finish gives every segment one lane) */
typedef struct nef_trust_args {
    const int64_t* seg_end;        /* [n_segs] device int64: the exclusive end of each segment in flat order, ascending, the last one = n */
    const float* seg_wd_mul;       /* [n_segs] device floats >= 0: the decay multiplier of the segment */
    const float* seg_adapt;        /* [n_segs] device floats: 0 = q_s is 1 (exempt), else the segment takes its trust ratio */
    float* ratio;                  /* [n_segs] caller-owned device table, out: the q_s of this call */
    float* stats;                  /* 4 caller-owned device words, see above */
    float* taint;                  /* NULL, or the device word in front of the flat gradients (the skip word of the update) */
    void* ws;                      /* device workspace, 8-byte aligned */
    size_t ws_bytes;
    float trust_coef;              /* rule 0: LARS's coefficient (>= 0).  Rule 1: unused */
    float trust_eps;               /* rule 0: added to LARS's denominator (>= 0).  Rule 1: unused */
    int32_t n_segs;                /* 1 .. NEF_TRUST_MAX_SEGS */
    int32_t reserved0;             /* 0 */
} nef_trust_args;

int nef_update_trust(const nef_update_args* a, const nef_trust_args* t, const nef_ema_args* e /* NULL: no average */,
                     nef_stream_t stream);
/* The workspace of one call over n elements in n_segs segments: the fp64 partial pairs of a grid that depends on n alone. */
size_t nef_update_trust_ws_bytes(int64_t n, int32_t n_segs);
/* sizeof(nef_trust_args) as the library was built. */
size_t nef_trust_args_bytes(void);
/* The per-update learning-rate schedule (no counterpart in the reference, whose two schedulers step per epoch): the effective rate of
 * an update is base * m(t), t = *t the number of updates APPLIED so far (the first update uses m(0)), with W = warmup_updates,
 * N = total_updates, s = warmup_start, f = lr_floor, p = poly_power:
 *   t < W:   m = s + (1 - s) * t / W                                            (torch's LinearLR, closed form)
 *   t >= W:  x = clamp((t - W) / max(1, N - W), 0, 1);
 *            shape 0 (const):  m = 1
 *            shape 1 (cosine): m = f + (1 - f) * (1 + cos(pi * x)) / 2         (CosineAnnealingLR, T_max = N - W, eta_min = f * base)
 *            shape 2 (poly):   m = f + (1 - f) * (1 - x)^p                     (PolynomialLR when f = 0)
 *   and m keeps its end value for t >= N.  N <= W: the span counts as 1 (x = 0 at t = W, 1 behind it); W = 0: no warm-up, no division.
 * m and the product are formed in fp64 and rounded ONCE into the fp32 word *lr_out -- the word the update entries take as lr_dev.
 * base = *base_dev (a device fp64 word) when base_dev is given, else the scalar.  *t is an int64 word: a float count stops at 2^24.
 *   advance = 1: behind an update.  The update counted as applied unless *skip_if_positive > 0 or *flag > 0 (either may be NULL) --
 *                the rule and the words of the one-lane launches behind nef_adam / nef_update_trust (flag: the 4-byte word at
 *                ws + nef_update_trust_ws_bytes(n, n_segs) - 16 of the nef_update_trust call in front).  Applied: *t += 1, then
 *                *lr_out = (float)(base * m(*t)).  Not applied: *t and *lr_out keep their bits.
 *   advance = 0: only *lr_out = (float)(base * m(*t)); *t is not written, the two words are not read.
 * One single-wave launch, lane 0 working.  args, t or lr_out NULL: NEF_E_NULL; shape outside 0..2: NEF_E_UNSUPPORTED; advance not 0 / 1,
 * a negative W or N, s or f outside [0, 1], p <= 0, a negative scalar base, or a NaN / infinity in any of them: NEF_E_SHAPE.  Every check
 * sits in front of the launch.  Capturable: nothing is read by the host, nothing is allocated. */
typedef struct nef_lr_sched_args {
    int64_t* t;                    /* device int64 word: applied updates */
    const double* base_dev;        /* NULL, or a device fp64 word that replaces `base` at run time */
    float* lr_out;                 /* device fp32 word, out: the rate of the next update */
    const float* skip_if_positive; /* NULL, or the skip word of the update in front */
    const float* flag;             /* NULL, or the trust flag of the nef_update_trust call in front */
    int64_t warmup_updates;        /* W >= 0 */
    int64_t total_updates;         /* N >= 0 */
    double base;                   /* the base rate when base_dev is NULL (>= 0) */
    double warmup_start;           /* s in [0, 1] */
    double lr_floor;               /* f in [0, 1] */
    double poly_power;             /* p > 0 */
    int32_t shape;                 /* 0 const, 1 cosine, 2 poly */
    int32_t advance;               /* 0 / 1 */
} nef_lr_sched_args;

int nef_lr_sched(const nef_lr_sched_args* a, nef_stream_t stream);
/* sizeof(nef_lr_sched_args) as the library was built. */
size_t nef_lr_sched_args_bytes(void);
/* Global gradient-norm clipping over a flat buffer: torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) on the averaged
 * gradient gscale * g (no counterpart in the reference).  total = gscale * sqrt(sum g[i]^2), coef = min(1, max_norm / (total + 1e-6)),
 * g[i] *= coef; g stays the un-averaged sum, so the update launch behind this call still applies gscale.  The sum is deterministic:
 * fp64 partial sums over a grid that depends on n alone and a one-block finish, no atomics -- the same buffer gives the same bits
 * eagerly, under hipGraph replay and on every rank.  Three launches; the scale pass takes 16-byte accesses from the first 16-byte
 * boundary of g on and returns without touching g when coef == 1.
 *   stats[0] = total of this call; stats[1] = the coefficient applied by this call (1 when g is left as it is);
 *   stats[2] += 1 when coef < 1; stats[3] += 1 when total is not finite.
 * A non-finite total leaves g as it is and, if `taint` is given, adds 1 to taint[0]: nef_sgd_momentum / nef_adam behind this call
 * (skip_if_positive = taint) then skip the step as they do for a tainted split-fp16 step.  This is a deliberate difference from
 * torch, whose clip_grad_norm_ multiplies by a NaN coefficient and so writes NaN into every parameter.  taint[0] > 0 on entry (the
 * step is skipped anyway): g, stats[2] and stats[3] stay as they are.  max_norm = +inf is legal (the norm is measured, nothing is ever
 * scaled); max_norm <= 0 or NaN returns NEF_E_SHAPE.  Capturable: nothing is read by the host, nothing is allocated. */
size_t nef_grad_clip_ws_bytes(void);
int nef_grad_clip(float* g, int64_t n, float max_norm, float gscale,
                  float* taint /* NULL, or the device word in front of the flat gradients (nef_h2_taint's output) */,
                  float* stats /* 4 device floats */, void* ws, size_t ws_bytes, nef_stream_t stream);
/* The split-fp16 convolutions (conv args wino = 3, nef_bww_args form 3) count the waves that had to clamp an operand at fp16's
 * range in a device counter (x_clamped); such a launch's results are wrong.  nef_h2_taint writes out[0] = (float)(*clamped_total -
 * *mark) -- the clamps since the previous call -- and sets *mark = *clamped_total: called once per train step behind the backward
 * pass, its output word travels with the gradients (summed by the data-parallel all-reduce, so every rank sees a clamp on any rank)
 * and makes nef_sgd_momentum skip the update.  No counterpart in the reference (its fp32 nn.Conv1d cannot overflow at 65504,
 * codes/network/model_nefnet.py:18-21); capturable, nothing is read by the host. */
int nef_h2_taint(const int32_t* clamped_total, int32_t* mark, float* out, nef_stream_t stream);
/* choice[0..1] = (c1, c2), seed[0] = seed_value, by a launch that carries the values as kernel arguments: the per-step host
 * decisions of a replayed (hipGraph) train step -- the two Standin lead draws of codes/network/model_nefnet.py:154,156 and the
 * dropout seed -- reach the device words the captured kernels read without a blocking host-to-device copy. */
int nef_step_words(int32_t* choice, int64_t* seed, int c1, int c2, int64_t seed_value, nef_stream_t stream);
/* Once per forward pass over the table of split-fp16 call-site magnitudes (ops.amax_roll; no counterpart in the reference, whose
 * fp32 convs need no operand scale): cur[i] = nxt[i] where nxt[i] > 0 and (cur[i] <= 0, or nxt[i] > follow_up * cur[i], or
 * nxt[i] * follow_down < cur[i], or follow_always); then nxt[i] = 0.  One launch. */
int nef_amax_roll(float* cur, float* nxt, int n, float follow_up, float follow_down, int follow_always, nef_stream_t stream);
/* out = concatenation of the n device tensors srcs[k] (sizes[k] floats each), one launch per 64 tensors.  `srcs` / `sizes` are HOST
 * arrays.  Builds the flat gradient buffer FusedSGD / the data-parallel all-reduce work on (replaces the torch.cat of
 * codes/solver's per-parameter .grad tensors; optim_scheduler.py:10 steps them one by one). */
int nef_flatten(const float* const* srcs, const int64_t* sizes, int n, float* out, nef_stream_t stream);
/* nef_flatten with an accumulate form (gradient accumulation, SOLVER.accum_steps: the micro-batches of a window are summed in fp32 into
 * the one flat gradient buffer; the reference accumulates by leaving out zero_grad()).  With off_k the sum of sizes[0..k):
 *   out[off_k + i]  = srcs[k][i]   when not accumulating -- `out` is never read, it may hold anything;
 *   out[off_k + i] += srcs[k][i]   when accumulating (one fp32 add per element, one writer per element, no atomics).
 * `accumulate` is 0 or 1.  A non-NULL `accumulate_dev` is a DEVICE word (int32) that replaces `accumulate` when the launch runs (non-zero:
 * accumulate), so one captured launch serves the first and the later micro-batches of a window.  `srcs` / `sizes` are HOST arrays; one
 * launch per 64 tensors, the grid a function of the sizes alone.  A source of 0 elements may be NULL.  Every argument is checked before
 * the first launch: NULL srcs / sizes / out with n > 0 (or a NULL source of sizes[k] > 0) is NEF_E_NULL; n < 0, a negative size or
 * `accumulate` outside {0, 1} is NEF_E_SHAPE; n == 0 is NEF_OK and launches nothing. */
int nef_flatten_acc(const float* const* srcs, const int64_t* sizes, int n, float* out, int accumulate, const int32_t* accumulate_dev,
                    nef_stream_t stream);
/* n independent segment copies or sums in one launch per 64 segments (csrc/views.hip; the glue of the multi-view train step,
 * SOLVER.train_views, which the reference has no counterpart of: its forward takes one query angle per step):
 *   dsts[k][i]  = srcs[k][i]   for i < sizes[k], when `accumulate` is 0 -- dsts[k] is never read;
 *   dsts[k][i] += srcs[k][i]   when `accumulate` is 1 (one fp32 add per element).
 * One writer per element, no atomics; the grid is a function of n and the sizes alone, so the bits are the same eagerly, under graph
 * replay and on every rank.  `srcs` / `dsts` / `sizes` are HOST arrays of DEVICE pointers / float counts.  The pointers need only
 * 4-byte alignment (they are slices): a segment whose source and destination share their offset inside a 16-byte line moves its body
 * in 16-byte accesses between a scalar head and tail, any other segment is scalar.  OVERLAPPING SEGMENTS ARE NOT SUPPORTED: no
 * destination may overlap another destination or any source of the call (a source may appear in several segments).  A segment of 0
 * elements may have NULL pointers.  Every argument is checked before the first launch: NULL srcs / dsts / sizes with n > 0 (or a NULL
 * source or destination of sizes[k] > 0) is NEF_E_NULL; n < 0, a negative size or `accumulate` outside {0, 1} is NEF_E_SHAPE; n == 0 is
 * NEF_OK and launches nothing. */
int nef_copy_many(const float* const* srcs, float* const* dsts, const int64_t* sizes, int n, int accumulate, nef_stream_t stream);
/* w [Co][2 Cih][K] -> grouped [2 Co][Cih][K] (group = input-channel half: the first decoder conv runs once per distinct half,
 * DESIGN.md section 2; weight of codes/network/model_nefnet.py:18), inverse != 0: the other way (its gradient). */
int nef_regroup_halves(const float* src, float* dst, int Co, int Cih, int K, int inverse, nef_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Polyphase form of a K = 3 conv behind the x2 linear upsampling (codes/network/model_nefnet.py:101-105, nn.Upsample + DoubleConv's
 * first conv): output 2m + p is a K = 3 conv of the HALF-resolution input with phase weights W'_p.
 * nef_poly_weights: w [rows][Cig][3] -> wsyn [2 rows][Cig][3], row 2 r + p = W'_p of row r.
 * Backward-data through conv + upsampling in one pass at half resolution: nef_conv_fwd with pro_mode 4 (input = the
 * full-resolution gradient [B][G Cog][T] read as 2 Cog phase channels of length T / 2), weights = wsyn packed transposed / flipped,
 * output = the gradient wrt the half-resolution input; then nef_poly_bwd_edge adds the two row-end terms the phase form leaves out
 * (and their share of the BatchNorm-backward sums, into slot 0 of the sample: bnb_* as in nef_conv_args, NULL slots = none). */
/* out[b][c] = sum over the nslot slots of sample b of slots[c][b*nslot + s][0] (the word-0 sums a conv epilogue left, stats_mode 1). */
int nef_slots_to_rows(const float* slots, int nslot, float* out, int B, int C, nef_stream_t stream);
int nef_poly_weights(const float* w, float* wsyn, int rows, int Cig, int tile_Cr /* 0, or the channels per group (a multiple of 64):
                     rows in the TILE order of the polyphase forward launch, phase p of channel co of group g = row
                     g 2 Cr + (co / 64) 128 + ((co / 32) & 1) 64 + p 32 + co % 32 */, nef_stream_t stream);
/* Forward in polyphase form: nef_conv_fwd with pro_mode 8 (| 1: the BatchNorm affine + ReLU prologue) -- x the half-resolution input
 * [B][G Cin_g][T], weights = tile-ordered wsyn (Cout_g = 2 x channels), y [B][G Cout_g / 2][2 T], bias / stats only; then
 * nef_poly_fwd_edge corrects the first and the last output column (and slot 0 of the statistics) for the conv's zero padding. */
int nef_poly_fwd_edge(const float* x, const float* w, float* y, int B, int G, int Cr /* output channels per group */, int Cig,
                      int T /* length of y = 2 x length of x */, const float* pro_a, const float* pro_b, int pro_Bp, float* stats,
                      int nslot, float* xedge /* NULL, or [B][G Cig][2]: the prologue's output at positions 0 and T/2 - 1 */,
                      nef_stream_t stream);
int nef_poly_bwd_edge(const float* gy, const float* w /* [G Cog][Cig][3], the conv's own weight */, float* gx, int B, int G, int Cog,
                      int Cig, int T /* length of gy = 2 x length of gx */, const float* bnb_x, const float* bnb_mean,
                      const float* bnb_invstd, const float* bnb_a, const float* bnb_b, int bnb_Bp, float* bnb_slots, int nslot,
                      int gy_phase_major /* gy stored [B][G 2 Cog][T / 2] (nef_bn_bwd_args.phase_major) */, nef_stream_t stream);
/* PHASE-MAJOR gradients: nef_bn_relu_bwd with nef_bn_bwd_args.phase_major (forms 0 and 3) writes row r of its output as the two
 * half-length rows 2 r (even positions) and 2 r + 1 (odd positions) of a [.., 2 C, L / 2] tensor.  That is the operand the polyphase backward passes of the
 * conv behind the upsampling want: backward-data = a PLAIN nef_conv_fwd over it (weights nef_poly_weights, transposed / flipped)
 * + nef_poly_bwd_edge(gy_phase_major = 1); weight gradient = nef_conv_bwd_weight, form 3, with pro_mode 4 (| 1: affine prologue; bit 2 =
 * the half-resolution x window is continued with x[0] / x[T-1] at the row ends) giving gw2 [G 2 Cog][Cig][3], then
 * nef_poly_wgrad_fold: gw2 folded back onto the conv's own taps minus the row-end terms (xedge [B][G Cig][2] = the prologue's
 * output at the first / last position, written by nef_poly_fwd_edge). */
size_t nef_poly_wgrad_fold_ws_bytes(int B, int G, int Cog, int Cig);
int nef_poly_wgrad_fold(const float* gw2, const float* gy_pm, const float* xedge, float* gw, void* ws, size_t ws_bytes, int B, int G,
                        int Cog, int Cig, int T /* full-resolution length = 2 x the rows of gy_pm */, nef_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Test-phase metrics on the device.  Replaces PSNR / SSIM of codes/utils/mertic.py:7-32 as called from
 * codes/solver/solver.py:202-228: per (sample, view) row over the un-padded region [0, rois[i][6][0]) (whole row
 * when rois is NULL).  pred, gt fp32 [B][Q][L]; psnr, ssim fp64 [B][Q].  PSNR = 100 for an exact match, else
 * 20*log10(1/rmse).  SSIM = skimage structural_similarity(data_range=1.0) for 1-D input (7-tap uniform window,
 * sample covariance, borders of 3 cropped); NaN for rows shorter than 7 (skimage raises there). */
int nef_view_metrics(const float* pred, const float* gt, const int64_t* rois, double* psnr, double* ssim, int B, int Q,
                     int L, nef_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Half-precision panorama decoder (BASELINE configs 4/5): the eval-mode view sweep of
 * model_nefnet.py:181-190 / gen_ecg :196-218 with BatchNorm folded into the convs (nef_fold_bn), activations kept
 * as fp16 [pair][time][channel] and the four wide decoder convs (model_nefnet.py:18,21 inside :103,:105) on the
 * fp16 matrix cores with fp32 accumulation.  No reference counterpart in reduced precision: gated against the fp32
 * path (2e-3 rel-L2).  Pairs are (sample, angle), sample-major: pair n = b*nq + i.
 * nef_pano_h_from_f32 : x fp32 [B][C][T] -> y fp16 [B][T][C].
 * nef_pano_h_pack_weight: w fp32 [Cout][Cin][3] (BN already folded) -> fp16 MFMA A-fragment order, Cout*Cin*3 halfs.
 * nef_pano_h_conv     : y[n] = ReLU(conv_k3_pad1(pro(x[n / x_div])) + bias), x fp16 [.][Tin][Cin], y fp16 [N][T][Cout];
 *                       pro_mode bit0: channel ci times scale[(n/nq)*sc_bs + (n%nq)*sc_is + ci] (fp32; the query
 *                       encoding q of model_nefnet.py:184-186), bit1: x2 linear upsample along time (Tin = T/2,
 *                       nn.Upsample align_corners=False, :102,:104).  (Cin,Cout) in {(256,128),(128,128),(128,64),(64,64)}.
 * nef_pano_h_outconv  : out[(n/nq)*out_bs + (n%nq)*out_is + t] = sigmoid((conv_k3(x[n]; w [1][64][3]) + bias)/3),
 *                       x fp16 [N][T][64], out fp32 (model_nefnet.py:106 + :186). */
int nef_pano_h_from_f32(const float* x, void* y, int B, int C, int T, nef_stream_t stream);
int nef_pano_h_pack_weight(const float* w, void* wp, int Cout, int Cin, nef_stream_t stream);
int nef_pano_h_conv(const void* x, const void* wp, const float* bias, const float* scale, void* y, int N, int T, int Cin,
                    int Cout, int pro_mode, int x_div, int nq, int64_t sc_bs, int64_t sc_is, nef_stream_t stream);
 /* nef_pano_h_conv_pair: layers 1 and 2 of the decoder (model_nefnet.py:102-103: Upsample, DoubleConv(256,128)) in one
 * pass (T even; up to 256 output rows one tile per pair, longer sequences -- round 6 -- in tiles of 252 output rows with recomputed
 * halo slots):
 *   y[n] = ReLU(conv_k3(ReLU(conv_k3(scale[n] * up2(x[n / x_div])) + bias1)) + bias2),  x fp16 [.][T/2][256],
 * y fp16 [N][T][128]; the 128-channel intermediate stays on chip and is rounded to fp16 exactly as the two-call
 * sequence nef_pano_h_conv(pro_mode 3) + nef_pano_h_conv(pro_mode 0) rounds it (bit-identical results). */
/* nef_pano_h_conv_tail (round 6): layers 3 and 4, the last conv and sigmoid(x/3) of the decoder (model_nefnet.py:104-106, :186) in
 * one pass (T even; up to 512 output rows one tile per pair, longer sequences in tiles of 508 output rows with recomputed halo slots):
 *   out[(n/nq)*out_bs + (n%nq)*out_is + t] = sigmoid((conv_k3(ReLU(conv_k3(ReLU(conv_k3(up2(x[n])) + bias3)) + bias4); wout) + bout) / 3),
 * x fp16 [N][T/2][128] (layer 2's output), wp3 / wp4 = nef_pano_h_pack_weight of the folded 128->64 / 64->64 weights, wout fp32
 * [1][64][3].  The two 64-channel intermediates stay on chip, rounded to fp16 exactly as nef_pano_h_conv(pro_mode 2) +
 * nef_pano_h_conv_outconv round them. */
int nef_pano_h_conv_tail(const void* x, const void* wp3, const float* bias3, const void* wp4, const float* bias4, const float* wout,
                         const float* bout, float* out, int N, int T, int nq, int64_t out_bs, int64_t out_is, nef_stream_t stream);
int nef_pano_h_conv_pair(const void* x, const void* wp1, const float* bias1, const float* scale, const void* wp2,
                         const float* bias2, void* y, int N, int T, int x_div, int nq, int64_t sc_bs, int64_t sc_is,
                         nef_stream_t stream);
 /* nef_pano_h_conv_outconv: the 64->64 layer and the last conv in one pass: out = sigmoid((conv_k3(ReLU(conv_k3(x) +
 * bias); wout) + bout)/3); the 64-channel intermediate never reaches memory (it is rounded to fp16 exactly as the
 * two-call sequence nef_pano_h_conv + nef_pano_h_outconv rounds it). */
int nef_pano_h_conv_outconv(const void* x, const void* wp, const float* bias, const float* wout, const float* bout,
                            float* out, int N, int T, int nq, int64_t out_bs, int64_t out_is, nef_stream_t stream);
int nef_pano_h_outconv(const void* x, const float* w, const float* bias, float* out, int N, int T, int nq,
                       int64_t out_bs, int64_t out_is, nef_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NEFNET_HIP_H */
