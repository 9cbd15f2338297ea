// Device helpers of the segment un-pooling (roi_pooling_1d.py:72-99) shared by roi.hip and the kernels that un-pool while they
// mix (the z2 halves of nef_lead_mean_mix_unpool / nef_mix_bwd_unpool): every kernel that evaluates the resampling or its
// transpose goes through the functions below, so their results agree bit for bit (the library is built with -ffp-contract=off).
#pragma once
#include "nef_common.h"

namespace nef_unpool {

constexpr int NSEG = NEF_N_SEG;
constexpr int BINS = NEF_ROI_BINS;
constexpr int SEGW = 2 * NEF_ROI_BINS;   // 32 samples per decoded segment

__device__ __forceinline__ int64_t latent_index(int64_t roi) {
    return (int64_t)((float)roi * 0.25f);   // rois.float().mul_(0.25).long()  (:82-85)
}

struct SegTable { int start[NSEG]; int len[NSEG]; int off[NSEG]; float scale[NSEG]; };

__device__ __forceinline__ bool load_segments(const int64_t* __restrict__ roi_b, int T, SegTable& st) {
    int run = 0;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NSEG; ++j) {
        const int64_t a = latent_index(roi_b[2 * j]);
        const int64_t e = latent_index(roi_b[2 * j + 1]);
        int64_t len = e - a;
        if (len < 0) { ok = false; len = 0; }
        if (run + len > T) { ok = false; len = T - run; }
        st.start[j] = (int)a;
        st.len[j] = (int)len;
        st.off[j] = run;
        st.scale[j] = len > 0 ? (float)SEGW / (float)(int)len : 0.f;      // F.interpolate's input/output ratio
        run += (int)len;
    }
    if (run != T) ok = false;
    return ok;
}

// F.interpolate(mode='linear', align_corners=False) source index for output i of a len-long segment
__device__ __forceinline__ void lerp_src(int i, float scale, int& i0, int& i1, float& l0, float& l1) {
    float src = scale * ((float)i + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = (int)src;
    if (i0 > SEGW - 1) i0 = SEGW - 1;
    i1 = i0 + (i0 < SEGW - 1 ? 1 : 0);
    l1 = src - (float)i0;
    if (l1 < 0.f) l1 = 0.f;
    if (l1 > 1.f) l1 = 1.f;
    l0 = 1.f - l1;
}

// the un-pooled value from lerp_src's two taps
__device__ __forceinline__ float unpool_lerp(float l0, float v0, float l1, float v1) { return l0 * v0 + l1 * v1; }

// first output i in [0, len] of a segment whose source index i0(i) reaches s (i0 is non-decreasing in i): the closed form
// of lerp_src's `scale*(i+0.5)-0.5 >= s`, then corrected by evaluating lerp_src itself around the guess, so that the
// transpose partitions the outputs exactly as the forward assigned them whatever the rounding of the closed form.
// lerp_src's left tap alone (its clamp to 31 does not matter against s <= 31)
__device__ __forceinline__ int unpool_left_tap(int i, float scale) {
    float src = scale * ((float)i + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    return (int)src;
}

__device__ __forceinline__ int unpool_first_reaching(int s, int len, float scale, float inv_scale) {
    if (s <= 0) return 0;
    int i = (int)ceilf(((float)s + 0.5f) * inv_scale - 0.5f);
    if (i < 0) i = 0;
    if (i > len) i = len;
    // the closed form and the forward's rounded expression can disagree by one position when the boundary falls within
    // rounding of an integer: one verified step either way ...
    if (i > 0 && unpool_left_tap(i - 1, scale) >= s) --i;
    else if (i < len && unpool_left_tap(i, scale) < s) ++i;
    // ... and, should that ever not be enough, the plain search (never taken in practice; keeps the partition exact)
    if ((i > 0 && unpool_left_tap(i - 1, scale) >= s) || (i < len && unpool_left_tap(i, scale) < s)) {
#pragma nounroll
        while (i > 0 && unpool_left_tap(i - 1, scale) >= s) --i;
#pragma nounroll
        while (i < len && unpool_left_tap(i, scale) < s) ++i;
    }
    return i;
}

// gather form of the transpose for one row `gr` (T gradients, global memory or an LDS strip): lane s of segment j collects the
// outputs that read sample s:
//   gz[j][s] = sum_{i: i0(i)=s} l0(i) g[i] + sum_{i: i1(i)=s} l1(i) g[i],  {i0 = s} = [first(s), first(s+1)),
//   {i1 = s} = {i0 = s-1} (plus {i0 = 31} for s = 31, where i1 is clamped) -- two short contiguous ranges instead of a
//   widened candidate window with a test per candidate (VALU-bound before: 985 vector instructions per element).
// Two segments per trip: lanes 0..31 and 32..63.  acc[k] is the lane's sum for segment 2k + (lane >> 5); the lanes of the
// upper half leave acc[3] (segment 7) untouched.
__device__ __forceinline__ void unpool_gather_row(const float* gr, const SegTable& st, int lane, float (&acc_out)[(NSEG + 1) / 2]) {
    const int s = lane & (SEGW - 1), half = lane >> 5;
#pragma unroll
    for (int jj = 0; jj < NSEG + 1; jj += 2) {
        const int j = jj + half;
        if (j >= NSEG) continue;
        const int len = half ? st.len[jj + 1 < NSEG ? jj + 1 : jj] : st.len[jj];
        const int off = half ? st.off[jj + 1 < NSEG ? jj + 1 : jj] : st.off[jj];
        const float sc = half ? st.scale[jj + 1 < NSEG ? jj + 1 : jj] : st.scale[jj];
        float acc = 0.f;
        if (len > 0) {
            const int b0 = unpool_first_reaching(s, len, sc, (float)len * (1.f / SEGW));
            const int nb = __shfl_down(b0, 1), pb = __shfl_up(b0, 1);   // neighbours lie in the same 32-lane half
            const int b1 = s + 1 < SEGW ? nb : len;
            const int a0 = s > 0 ? pb : b0;
            // outputs in [a0, b0) read s as their RIGHT tap: weight l1 = src - (s - 1), in [0, 1) without a clamp because
            // their left tap is s - 1; outputs in [b0, b1) read it as their LEFT tap: weight l0 = 1 - (src - s) -- and at
            // s = 31 the right tap is clamped onto the left one, the two weights add up to 1.  src is lerp_src's
            // expression term for term ((float)i + 0.5f is exact, so the running fi below is too).
            const float* gp = gr + off;
            float fi = (float)a0 + 0.5f;
            const float sm1 = (float)(s - 1);
            for (int i = a0; i < b0; ++i, fi += 1.f) {
                float src = sc * fi - 0.5f;
                src = src < 0.f ? 0.f : src;
                acc += (src - sm1) * gp[i];
            }
            const float c0 = s == SEGW - 1 ? 1.f : (float)(s + 1), k = s == SEGW - 1 ? 0.f : 1.f;
            for (int i = b0; i < b1; ++i, fi += 1.f) {
                float src = sc * fi - 0.5f;
                src = src < 0.f ? 0.f : src;
                acc += (c0 - k * src) * gp[i];
            }
        }
        acc_out[jj >> 1] = acc;
    }
}

}  // namespace nef_unpool

// Cross-file launchers of the un-pooling mixes (entries in elementwise.hip, z2 halves in roi.hip).
// z2 half of nef_lead_mean_mix_unpool: latent / D2 rows 128..255 from the segment tensor z2b [B][128V][7][32]
NEF_HIDDEN void nef_unpool_mix_fwd_z2(const float* z2b, const int64_t* rois, const float* q, float* latent, float* D2, int32_t* status,
                                      int B, int V, int T, int c2, const int32_t* choice_dev, hipStream_t st);
// z2 half of nef_mix_bwd_unpool: gz2b [B][128V][7][32] and gq rows 128..255 from gD [2B][256][T].  group: positions per lane and
// trip of the nef_mix_bwd kernel the z1 half runs (4: the row-pair kernel, T % 4 == 2; 2: position pairs, T even; 1: scalar) --
// the z2 half deals its positions to the lanes the same way, which keeps gq's summation order
NEF_HIDDEN void nef_unpool_mix_bwd_z2(const float* gD, const float* latent, const float* z2b, const int64_t* rois, const float* q,
                                      float* gz2b, float* gq, int B, int V, int T, int c2, const int32_t* choice_dev, int group,
                                      hipStream_t st);
