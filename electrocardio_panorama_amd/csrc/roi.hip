// Heartbeat-segment ROI ops on the latent time axis.
//   roi_align : reference codes/network/utils/roi_pooling_1d.py:38-69 (`roi_algin`).  The reference feeds
//               F.grid_sample a [B,C,T,1] image and a grid whose x component carries the ROI positions, so x
//               addresses the size-1 axis and y = 0 addresses the middle of time.  This kernel
//               evaluates exactly that bilinear sample with zero padding, align_corners=False.
//   roi_unpool: roi_pooling_1d.py:72-99 (`roi_pooling_reverse`): per (sample, segment) linear resampling
//               32 -> len_j (align_corners=False) concatenated along time.  Integer bookkeeping (:82-92) is
//               (long)(float(roi) * 0.25f), bit-exact with the reference.
// rois stay int64 on the device; no host loop, no per-segment launches.
#include "nef_common.h"
#include "roi_unpool.h"

namespace {

using namespace nef_unpool;      // NSEG / BINS / SEGW, latent_index, SegTable, load_segments, lerp_src, unpool_lerp, the gather transpose

// grid x for (segment j, bin s): torch.linspace(r0, r1, 16) on fp32, r = roi*0.25*(2/T) - 1   (:50-58)
__device__ __forceinline__ float grid_x(const int64_t* __restrict__ roi_b, int j, int s, int T) {
    const float sc = (float)(2.0 / (double)T);
    const float r0 = ((float)roi_b[2 * j] * 0.25f) * sc + (-1.0f);
    const float r1 = ((float)roi_b[2 * j + 1] * 0.25f) * sc + (-1.0f);
    const float step = (r1 - r0) / (float)(BINS - 1);
    return s < BINS / 2 ? r0 + step * (float)s : r1 - step * (float)(BINS - 1 - s);
}

// bilinear weight of the single column (W == 1) for normalised x, zero padding
__device__ __forceinline__ float col_weight(float gx) {
    const float ix = ((gx + 1.f) * 1.f - 1.f) * 0.5f;
    const float x0 = floorf(ix);
    const float we = ix - x0;          // weight of column x0+1
    const float ww = 1.f - we;         // weight of column x0
    float w = 0.f;
    if (x0 == 0.f) w += ww;
    if (x0 + 1.f == 0.f) w += we;
    return w;
}

struct RowTap { int r0, r1; float w0, w1; };

__device__ __forceinline__ RowTap row_taps(int T) {
    const float iy = ((0.f + 1.f) * (float)T - 1.f) * 0.5f;
    const float y0 = floorf(iy);
    RowTap rt;
    rt.r0 = (int)y0;
    rt.r1 = rt.r0 + 1;
    rt.w1 = iy - y0;
    rt.w0 = 1.f - rt.w1;
    if (rt.r0 < 0 || rt.r0 >= T) rt.w0 = 0.f;
    if (rt.r1 < 0 || rt.r1 >= T) { rt.w1 = 0.f; rt.r1 = rt.r0; }
    if (rt.r0 < 0 || rt.r0 >= T) rt.r0 = rt.r1;
    return rt;
}

// one thread per output element; out [B][C][7][16]
// z may hold only a window of the time axis: zT stored samples per row starting at time t_off (the two rows read
// are the only ones roi_algin ever touches, so the producer can skip the rest -- see engine.py).
__global__ void roi_align_fwd_kernel(const float* __restrict__ z, const int64_t* __restrict__ rois,
                                     float* __restrict__ out, int B, int C, int T, int zT, int t_off) {
    const int64_t n = (int64_t)B * C * NSEG * BINS;
    const RowTap rt = row_taps(T);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int s = (int)(i % BINS);
        const int j = (int)((i / BINS) % NSEG);
        const int64_t bc = i / (BINS * NSEG);
        const int b = (int)(bc / C);
        const float wx = col_weight(grid_x(rois + (int64_t)b * NSEG * 2, j, s, T));
        const float* zr = z + bc * zT - t_off;
        // grid_sample accumulates nw*(n*w) + ne*.. + sw*(s*w) + se*..; with W == 1 only one column is in range
        out[i] = zr[rt.r0] * (rt.w0 * wx) + zr[rt.r1] * (rt.w1 * wx);
    }
}

// gz [B][C][T]: zero except the two middle rows
__global__ void roi_align_bwd_kernel(const float* __restrict__ gout, const int64_t* __restrict__ rois,
                                     float* __restrict__ gz, int B, int C, int T, int zT, int t_off) {
    const int64_t rows = (int64_t)B * C;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const RowTap rt = row_taps(T);
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const int b = (int)(row / C);
        float acc = 0.f;
        for (int e = lane; e < NSEG * BINS; e += 64) {
            const int j = e / BINS, s = e % BINS;
            const float wx = col_weight(grid_x(rois + (int64_t)b * NSEG * 2, j, s, T));
            acc = fmaf(gout[row * NSEG * BINS + e], wx, acc);
        }
        acc = nef_wave_sum(acc);
        float* gr = gz + row * zT - t_off;
        for (int t = t_off + lane; t < t_off + zT; t += 64) {
            float v = 0.f;
            if (t == rt.r0) v += acc * rt.w0;
            if (t == rt.r1 && rt.w1 != 0.f) v += acc * rt.w1;
            gr[t] = v;
        }
    }
}

// one wave per (b, c) row of the output; zseg [B][C][7][32] -> out [B][C][T].
// The pass is VALU-bound, not HBM-bound (PMC: 1.7e8 vector instructions for 1.2e8 outputs in the first version, which
// searched the segment of every output with a 7-way select chain): the wave therefore walks the row SEGMENT BY SEGMENT --
// the segment's offset, length and scale are wave-uniform (scalar registers), a lane only evaluates lerp_src for its
// own output and gathers two of the segment's 32 samples.
__global__ void roi_unpool_fwd_kernel(const float* __restrict__ zseg, const int64_t* __restrict__ rois,
                                      float* __restrict__ out, int32_t* __restrict__ status, int B, int C, int T) {
    const int64_t rows = (int64_t)B * C;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    // a wave takes a contiguous run of rows: they mostly belong to one sample, whose segment table (about 70 vector
    // instructions per segment: i64 <-> f32 conversions and a division) is then derived once, not once per row
    const int64_t per_wave = (rows + (int64_t)gridDim.x * 4 - 1) / ((int64_t)gridDim.x * 4);
    const int64_t row_lo = ((int64_t)blockIdx.x * 4 + wave) * per_wave;
    const int64_t row_hi = row_lo + per_wave < rows ? row_lo + per_wave : rows;
    int b_cur = -1;
    SegTable st;
    for (int64_t row = row_lo; row < row_hi; ++row) {
        const int b = (int)(row / C);
        if (b != b_cur) {
            b_cur = b;
            const bool ok = load_segments(rois + (int64_t)b * NSEG * 2, T, st);
            if (!ok && status && lane == 0) status[0] = 1;
        }
        const float* zr = zseg + row * NSEG * SEGW;
        float* orow = out + row * T;
        // the row's 7 x 32 samples live in four registers of the wave (sample e in register e / 64, lane e % 64); the two
        // taps of an output come over the cross-lane network (ds_bpermute) instead of two dependent memory gathers
        float r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = (q * 64 + lane < NSEG * SEGW) ? zr[q * 64 + lane] : 0.f;
        int covered = 0;
#pragma unroll
        for (int j = 0; j < NSEG; ++j) {
            const int len = st.len[j], off = st.off[j];
            const float sc = st.scale[j];
            const float reg = r[j >> 1];
            const int base = (j & 1) * SEGW;
            for (int ib = 0; ib < len; ib += 64) {                 // wave-uniform trip count: every lane feeds the shuffles
                const int i = ib + lane;
                int i0, i1;
                float l0, l1;
                lerp_src(i, sc, i0, i1, l0, l1);
                const float v0 = __shfl(reg, base + i0), v1 = __shfl(reg, base + i1);
                if (i < len) orow[off + i] = unpool_lerp(l0, v0, l1, v1);
            }
            covered = off + len;
        }
        for (int t = covered + lane; t < T; t += 64) orow[t] = 0.f;     // segments that do not reach T (flagged in status)
    }
}

// the transpose of the above, in its gather form (unpool_gather_row).
// STAGED = true: the wave first streams its gradient row into a private LDS strip (coalesced, all loads in flight at
// once), then gathers from LDS -- the strided global gathers of the direct form are latency-bound (PMC: 60 % of wave
// cycles parked).  STAGED = false reads the row in place and serves rows too long for the strip (T > 4096).
template <bool STAGED>
__global__ __launch_bounds__(256) void roi_unpool_bwd_kernel(const float* __restrict__ gout,
                                                             const int64_t* __restrict__ rois,
                                                             float* __restrict__ gzseg, int B, int C, int T) {
    extern __shared__ float strip_lds[];
    const int64_t rows = (int64_t)B * C;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int s = lane & (SEGW - 1), half = lane >> 5;          // two segments per trip: lanes 0..31 and 32..63
    const int64_t per_wave = (rows + (int64_t)gridDim.x * 4 - 1) / ((int64_t)gridDim.x * 4);     // see the forward
    const int64_t row_lo = ((int64_t)blockIdx.x * 4 + wave) * per_wave;
    const int64_t row_hi = row_lo + per_wave < rows ? row_lo + per_wave : rows;
    int b_cur = -1;
    SegTable st;
    for (int64_t row = row_lo; row < row_hi; ++row) {
        const int b = (int)(row / C);
        if (b != b_cur) {
            b_cur = b;
            load_segments(rois + (int64_t)b * NSEG * 2, T, st);
        }
        const float* grow = gout + row * T;
        const float* gr = grow;
        if constexpr (STAGED) {
            float* strip = strip_lds + wave * T;
            // NU loads per lane in flight at once: a T = 1250 row (20 x 64 floats) is one trip -- with 5 per trip the wave
            // paid four HBM round trips per row (33 % of the HBM roof, round 2)
            constexpr int NU = 20;
            for (int t0 = 0; t0 < T; t0 += 64 * NU) {
                float v[NU];
#pragma unroll
                for (int u = 0; u < NU; ++u) v[u] = (t0 + u * 64 + lane < T) ? grow[t0 + u * 64 + lane] : 0.f;
#pragma unroll
                for (int u = 0; u < NU; ++u)
                    if (t0 + u * 64 + lane < T) strip[t0 + u * 64 + lane] = v[u];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            gr = strip;
        }
        float* gz = gzseg + row * NSEG * SEGW;
        float acc[(NSEG + 1) / 2] = {0.f, 0.f, 0.f, 0.f};
        unpool_gather_row(gr, st, lane, acc);
#pragma unroll
        for (int k = 0; k < (NSEG + 1) / 2; ++k)
            if (2 * k + half < NSEG) gz[(2 * k + half) * SEGW + s] = acc[k];
        if constexpr (STAGED) __builtin_amdgcn_wave_barrier();     // the strip is rewritten by the next row
    }
}

// The segment an output position t falls into (the forward's partition of [0, T): segment j owns [off_j, off_j + len_j), empty
// segments own nothing): i = position inside it, sc = its scale, jb = index of its first sample in a lead's 7 x 32 samples.
// Returns false for positions the segments do not reach.  The table is wave-uniform, a lane pays six compares.
__device__ __forceinline__ bool segment_of(const SegTable& st, int t, int& i, float& sc, int& jb) {
    int off = st.off[0];
    sc = st.scale[0];
    jb = 0;
#pragma unroll
    for (int j = 1; j < NSEG; ++j)
        if (t >= st.off[j]) { off = st.off[j]; sc = st.scale[j]; jb = j * SEGW; }
    i = t - off;
    return t < st.off[NSEG - 1] + st.len[NSEG - 1];
}

// z2 half of nef_lead_mean_mix_unpool = roi_unpool_fwd_kernel + the rows c >= 128 of lead_mean_mix_shared_kernel without the
// un-pooled tensor between them.  One wave per (b, c): the V leads' 7 x 32 segment samples sit in a per-wave LDS strip
// (V * 896 bytes), the wave streams over the output row, W positions per lane; lerp_src runs once per position (the segment table
// belongs to the sample, not to the lead) and every lead's value is unpool_lerp of its own two taps -- the expressions and the
// order of roi_unpool_fwd_kernel and lead_mean_mix_shared_kernel (s = v0; s += v_v; m = s / fv), so latent and D2 come out bit
// for bit; positions the segments do not reach carry the zeros the two kernels would have passed on.
template <int W>
__global__ __launch_bounds__(256) void unpool_mix_fwd_z2_kernel(const float* __restrict__ z2b, const int64_t* __restrict__ rois,
                                                                const float* __restrict__ q, float* __restrict__ latent,
                                                                float* __restrict__ D2, int32_t* __restrict__ status, int B, int V,
                                                                int T, int c2, const int32_t* __restrict__ choice_dev) {
    typedef float vec __attribute__((ext_vector_type(W)));
    extern __shared__ float strip_lds[];
    constexpr int ROW = NSEG * SEGW;
    if (choice_dev) c2 = choice_dev[1];
    const int64_t rows = (int64_t)B * 128;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int64_t per_wave = (rows + (int64_t)gridDim.x * 4 - 1) / ((int64_t)gridDim.x * 4);     // see roi_unpool_fwd_kernel
    const int64_t row_lo = ((int64_t)blockIdx.x * 4 + wave) * per_wave;
    const int64_t row_hi = row_lo + per_wave < rows ? row_lo + per_wave : rows;
    float* strip = strip_lds + wave * V * ROW;
    const int n = V * ROW;
    const float fv = (float)V;
    const int64_t pass = (int64_t)B * 256 * T;
    int b_cur = -1;
    SegTable st;
    for (int64_t row = row_lo; row < row_hi; ++row) {
        const int b = (int)(row >> 7), c = (int)(row & 127);
        if (b != b_cur) {
            b_cur = b;
            const bool ok = load_segments(rois + (int64_t)b * NSEG * 2, T, st);
            if (!ok && status && lane == 0) status[0] = 1;
        }
        // lead v's samples of this (b, c): z2b row (b*V + v)*128 + c; NU loads per lane in flight per trip
        const float* zr = z2b + ((int64_t)b * V * 128 + c) * ROW;
        constexpr int NU = 8;
        for (int e0 = 0; e0 < n; e0 += 64 * NU) {
            float r[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int e = e0 + u * 64 + lane, v = e / ROW;
                r[u] = e < n ? zr[(int64_t)v * 128 * ROW + (e - v * ROW)] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < NU; ++u)
                if (e0 + u * 64 + lane < n) strip[e0 + u * 64 + lane] = r[u];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int64_t orow = ((int64_t)b * 256 + 128 + c) * T;
        const float f = q[b * 256 + 128 + c];
        for (int p = lane; p < T / W; p += 64) {
            vec m, dm, dp;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                int i, jb;
                float sc;
                const bool in = segment_of(st, W * p + w, i, sc, jb);
                int i0 = 0, i1 = 0;
                float l0 = 0.f, l1 = 0.f;
                if (in) lerp_src(i, sc, i0, i1, l0, l1);
                float sum = 0.f, pk = 0.f;
                for (int v = 0; v < V; ++v) {
                    const float val = in ? unpool_lerp(l0, strip[v * ROW + jb + i0], l1, strip[v * ROW + jb + i1]) : 0.f;
                    sum = v == 0 ? val : sum + val;
                    if (v == 0 || v == c2) pk = val;
                }
                const float mean = sum / fv;
                m[w] = mean;
                dm[w] = f * mean;
                dp[w] = f * pk;
            }
            *(vec*)(latent + orow + W * p) = m;
            *(vec*)(D2 + orow + W * p) = dm;
            *(vec*)(D2 + pass + orow + W * p) = dp;
        }
        __builtin_amdgcn_wave_barrier();     // the strip is rewritten by the next row
    }
}

// z2 half of nef_mix_bwd_unpool = the rows c >= 128 of mix_bwd_kernel<false, true> + roi_unpool_bwd_kernel<true> without the
// gradient gz2r between them.  One wave per (b, c).  Per wave in LDS: two T-long strips and the picked lead's 7 x 32 samples.
//   1. stream the rows ga, gb of gD and the latent row (coalesced, NU of each in flight); per position form mix_bwd's two DISTINCT
//      output rows in the strips: everyone's f*ga/fv + 0 and the picked lead's f*ga/fv + f*gb (mix_bwd writes the first to V - 1
//      leads), and the row's gq term ga*lat + gb*pk, pk = the picked lead's un-pooled value rebuilt by the forward's functions;
//   2. unpool_gather_row once per strip; the picked lead's segment row takes the second result, every other lead's the first.
// G: how step 1 deals the row's positions to the lanes -- exactly as the nef_mix_bwd kernel that would have taken this row does, so
// that gq adds the same terms in the same order and comes out bit for bit as well: G = 4 mix_bwd_shared_pair_kernel (the row is half
// of an aligned span of four-float groups, an odd channel's row starts T floats into it, lane = group % 64), G = 2
// mix_bwd_kernel<false, true>'s vector path (position pairs), G = 1 its scalar path.  A lane adds its groups in ascending order.
template <int G>
__global__ __launch_bounds__(256) void unpool_mix_bwd_z2_kernel(const float* __restrict__ gD, const float* __restrict__ latent,
                                                                const float* __restrict__ z2b, const int64_t* __restrict__ rois,
                                                                const float* __restrict__ q, float* __restrict__ gz2b,
                                                                float* __restrict__ gq, int B, int V, int T, int c2,
                                                                const int32_t* __restrict__ choice_dev) {
    extern __shared__ float strip_lds[];
    constexpr int ROW = NSEG * SEGW;
    if (choice_dev) c2 = choice_dev[1];
    const int64_t rows = (int64_t)B * 128;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int s = lane & (SEGW - 1), half = lane >> 5;
    const int64_t per_wave = (rows + (int64_t)gridDim.x * 4 - 1) / ((int64_t)gridDim.x * 4);
    const int64_t row_lo = ((int64_t)blockIdx.x * 4 + wave) * per_wave;
    const int64_t row_hi = row_lo + per_wave < rows ? row_lo + per_wave : rows;
    float* sa = strip_lds + wave * (2 * T + ROW);
    float* sb = sa + T;
    float* pick = sb + T;
    const float fv = (float)V;
    const int64_t pass = (int64_t)B * 256 * T;
    int b_cur = -1;
    SegTable st;
    for (int64_t row = row_lo; row < row_hi; ++row) {
        const int b = (int)(row >> 7), c = (int)(row & 127);
        if (b != b_cur) {
            b_cur = b;
            load_segments(rois + (int64_t)b * NSEG * 2, T, st);
        }
        const float* zr = z2b + (((int64_t)b * V + c2) * 128 + c) * ROW;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u * 64 + lane < ROW) pick[u * 64 + lane] = zr[u * 64 + lane];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int64_t grow = ((int64_t)b * 256 + 128 + c) * T;
        const float f = q[b * 256 + 128 + c];
        float acc = 0.f;
        constexpr int NU = G == 4 ? 6 : (G == 2 ? 10 : 20);      // a T = 1250 row is one trip
        const int shift = G == 4 ? (c & 1) * T : 0;              // where the row starts in its span of groups
        const int kb = shift / G, ke = (shift + T + G - 1) / G;   // the groups that hold positions of this row
        for (int k0 = (kb & ~63) + lane; k0 < ke; k0 += 64 * NU) {
            float ga[NU][G], gb[NU][G], la[NU][G];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int k = k0 + 64 * u;
                if constexpr (G == 1) {
                    const bool in = k >= kb && k < ke;
                    ga[u][0] = in ? gD[grow + k] : 0.f;
                    gb[u][0] = in ? gD[pass + grow + k] : 0.f;
                    la[u][0] = in ? latent[grow + k] : 0.f;
                } else {
#pragma unroll
                    for (int e = 0; e < G; e += 2) {      // (T is even: a pair of positions is inside the row or outside it)
                        const int t = G * k + e - shift;
                        const bool in = k >= kb && k < ke && t >= 0 && t < T;
                        const nef_f32x2 z = {0.f, 0.f};
                        const nef_f32x2 a2 = in ? *(const nef_f32x2*)(gD + grow + t) : z;
                        const nef_f32x2 b2 = in ? *(const nef_f32x2*)(gD + pass + grow + t) : z;
                        const nef_f32x2 l2 = in ? *(const nef_f32x2*)(latent + grow + t) : z;
                        ga[u][e] = a2[0], ga[u][e + 1] = a2[1];
                        gb[u][e] = b2[0], gb[u][e + 1] = b2[1];
                        la[u][e] = l2[0], la[u][e + 1] = l2[1];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int k = k0 + 64 * u;
#pragma unroll
                for (int e = 0; e < G; ++e) {
                    const int t = G * k + e - shift;
                    if (k >= kb && k < ke && t >= 0 && t < T) {
                        int i, jb, i0, i1;
                        float sc, l0, l1, pk = 0.f;
                        if (segment_of(st, t, i, sc, jb)) {
                            lerp_src(i, sc, i0, i1, l0, l1);
                            pk = unpool_lerp(l0, pick[jb + i0], l1, pick[jb + i1]);
                        }
                        acc += ga[u][e] * la[u][e] + gb[u][e] * pk;
                        const float gm = f * ga[u][e] / fv;
                        sa[t] = gm + 0.f;
                        sb[t] = gm + f * gb[u][e];
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float ra[(NSEG + 1) / 2] = {0.f, 0.f, 0.f, 0.f}, rb[(NSEG + 1) / 2] = {0.f, 0.f, 0.f, 0.f};
        unpool_gather_row(sa, st, lane, ra);
        unpool_gather_row(sb, st, lane, rb);
        for (int v = 0; v < V; ++v) {
            float* gz = gz2b + (((int64_t)b * V + v) * 128 + c) * ROW;
#pragma unroll
            for (int k = 0; k < (NSEG + 1) / 2; ++k)
                if (2 * k + half < NSEG) gz[(2 * k + half) * SEGW + s] = v == c2 ? rb[k] : ra[k];
        }
        acc = nef_wave_sum(acc);
        if (lane == 0) gq[b * 256 + 128 + c] = acc;
        __builtin_amdgcn_wave_barrier();     // the strips are rewritten by the next row
    }
}

__global__ void roi_segment_table_kernel(const int64_t* __restrict__ rois, int64_t* __restrict__ seg_start,
                                         int64_t* __restrict__ seg_len, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t a = latent_index(rois[2 * i]);
    const int64_t e = latent_index(rois[2 * i + 1]);
    seg_start[i] = a;
    seg_len[i] = e - a;
}

}  // namespace

// the callers (elementwise.hip) have validated the arguments: 1 <= V <= NEF_UNPOOL_MIX_MAX_V, 2 <= T <= NEF_UNPOOL_MIX_MAX_T (backward)
void nef_unpool_mix_fwd_z2(const float* z2b, const int64_t* rois, const float* q, float* latent, float* D2, int32_t* status, int B,
                           int V, int T, int c2, const int32_t* choice_dev, hipStream_t st) {
    const dim3 grid(nef_stream_grid((int64_t)B * 128, 4));
    const size_t lds = (size_t)4 * V * NSEG * SEGW * sizeof(float);
    const bool al8 = (((uintptr_t)latent | (uintptr_t)D2) & 7) == 0;
    if (T % 2 == 0 && al8)
        hipLaunchKernelGGL(unpool_mix_fwd_z2_kernel<2>, grid, dim3(256), lds, st, z2b, rois, q, latent, D2, status, B, V, T, c2,
                           choice_dev);
    else
        hipLaunchKernelGGL(unpool_mix_fwd_z2_kernel<1>, grid, dim3(256), lds, st, z2b, rois, q, latent, D2, status, B, V, T, c2,
                           choice_dev);
}

void nef_unpool_mix_bwd_z2(const float* gD, const float* latent, const float* z2b, const int64_t* rois, const float* q, float* gz2b,
                           float* gq, int B, int V, int T, int c2, const int32_t* choice_dev, int group, hipStream_t st) {
    static_assert((size_t)4 * (2 * NEF_UNPOOL_MIX_MAX_T + NSEG * SEGW) * sizeof(float) <= 65536, "four waves' strips fit the default LDS limit");
    const size_t lds = (size_t)4 * (2 * T + NSEG * SEGW) * sizeof(float);
    const dim3 grid(nef_stream_grid((int64_t)B * 128, 4));
    if (group == 4)
        hipLaunchKernelGGL(unpool_mix_bwd_z2_kernel<4>, grid, dim3(256), lds, st, gD, latent, z2b, rois, q, gz2b, gq, B, V, T, c2, choice_dev);
    else if (group == 2)
        hipLaunchKernelGGL(unpool_mix_bwd_z2_kernel<2>, grid, dim3(256), lds, st, gD, latent, z2b, rois, q, gz2b, gq, B, V, T, c2, choice_dev);
    else
        hipLaunchKernelGGL(unpool_mix_bwd_z2_kernel<1>, grid, dim3(256), lds, st, gD, latent, z2b, rois, q, gz2b, gq, B, V, T, c2, choice_dev);
}

#define NEF_ST ((hipStream_t)stream)

extern "C" {

static bool window_covers_taps(int T, int zT, int t_off) {
    const int r0 = (T - 1) / 2, r1 = (r0 + 1 < T) ? r0 + 1 : r0;
    return zT > 0 && t_off >= 0 && t_off <= r0 && r1 < t_off + zT && t_off + zT <= T;
}

int nef_roi_align_fwd(const float* z, const int64_t* rois, float* out, int B, int C, int T, int zT, int t_off,
                      nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(z && rois && out, NEF_E_NULL);
    NEF_REQUIRE(B > 0 && C > 0 && T > 0 && window_covers_taps(T, zT, t_off), NEF_E_SHAPE);
    const int64_t n = (int64_t)B * C * NSEG * BINS;
    hipLaunchKernelGGL(roi_align_fwd_kernel, dim3(nef_stream_grid(n, 256)), dim3(256), 0, NEF_ST, z, rois, out, B, C, T,
                       zT, t_off);
    return nef_launch_status();
}

int nef_roi_align_bwd(const float* gout, const int64_t* rois, float* gz, int B, int C, int T, int zT, int t_off,
                      nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(gout && rois && gz, NEF_E_NULL);
    NEF_REQUIRE(B > 0 && C > 0 && T > 0 && window_covers_taps(T, zT, t_off), NEF_E_SHAPE);
    hipLaunchKernelGGL(roi_align_bwd_kernel, dim3(nef_stream_grid((int64_t)B * C, 4)), dim3(256), 0, NEF_ST, gout, rois,
                       gz, B, C, T, zT, t_off);
    return nef_launch_status();
}

int nef_roi_unpool_fwd(const float* zseg, const int64_t* rois, float* out, int32_t* status, int B, int C, int T,
                       nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(zseg && rois && out, NEF_E_NULL);
    NEF_REQUIRE(B > 0 && C > 0 && T > 0, NEF_E_SHAPE);
    hipLaunchKernelGGL(roi_unpool_fwd_kernel, dim3(nef_stream_grid((int64_t)B * C, 4)), dim3(256), 0, NEF_ST, zseg,
                       rois, out, status, B, C, T);
    return nef_launch_status();
}

int nef_roi_unpool_bwd(const float* gout, const int64_t* rois, float* gzseg, int B, int C, int T,
                       nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(gout && rois && gzseg, NEF_E_NULL);
    NEF_REQUIRE(B > 0 && C > 0 && T > 0, NEF_E_SHAPE);
    const dim3 grid(nef_stream_grid((int64_t)B * C, 4));
    if (T <= 4096)
        hipLaunchKernelGGL(roi_unpool_bwd_kernel<true>, grid, dim3(256), (size_t)4 * T * sizeof(float), NEF_ST, gout,
                           rois, gzseg, B, C, T);
    else
        hipLaunchKernelGGL(roi_unpool_bwd_kernel<false>, grid, dim3(256), 0, NEF_ST, gout, rois, gzseg, B, C, T);
    return nef_launch_status();
}

int nef_roi_segment_table(const int64_t* rois, int64_t* seg_start, int64_t* seg_len, int B, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(rois && seg_start && seg_len, NEF_E_NULL);
    NEF_REQUIRE(B > 0, NEF_E_SHAPE);
    const int n = B * NSEG;
    hipLaunchKernelGGL(roi_segment_table_kernel, dim3((n + 255) / 256), dim3(256), 0, NEF_ST, rois, seg_start, seg_len,
                       n);
    return nef_launch_status();
}

}  // extern "C"
