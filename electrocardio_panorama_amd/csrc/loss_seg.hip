// Wave-segment weights on the reconstruction term of the training loss (cfg.SOLVER.seg_weights) and the per-segment squared error of
// the test phase (cfg.SOLVER.seg_eval).  One definition of "the segment of a position", used by all three kernels (include/nefnet_hip.h,
// nef_loss_seg_args): end_i = clamp(rois[i, 6, 0], 0, L) -- nef_row_end of nef_common.h --; t >= end_i is segment 6 (pad); otherwise the
// segment is the number of k in 1..5 with rois[i, k, 0] <= t.  Only the six start points are read, so the rule is total for any int64
// content.  The starts are clamped to [0, L] once per block: for 0 <= t < L that keeps every comparison (s < 0 -> 0 <= t holds;
// s > L -> L <= t fails), and the per-element work is five 32-bit compares.  The weight of a position is picked by a select chain over
// that count -- no private array is indexed by a run-time value, so nothing lives in scratch.  Every sum has a fixed order (no atomics).
#include "nef_common.h"

namespace {

constexpr int TILE = NEF_LOSS_SEG_TILE;
static_assert(TILE == 256 * 4, "one float4 per thread of a 256-thread block");

// the six clamped boundaries of one row: s[0..4] = starts of segments 1..5, end = start of the padding
struct seg_row {
    int s1, s2, s3, s4, s5, end;
};

__device__ __forceinline__ int clamp_pos(int64_t v, int L) { return v < 0 ? 0 : (v > L ? L : (int)v); }

__device__ __forceinline__ seg_row load_row(const int64_t* __restrict__ rois, int i, int L) {
    const int64_t* r = rois + (int64_t)i * 14;          // rois[i, k, 0] = r[2 k]
    seg_row s;
    s.s1 = clamp_pos(r[2], L), s.s2 = clamp_pos(r[4], L), s.s3 = clamp_pos(r[6], L);
    s.s4 = clamp_pos(r[8], L), s.s5 = clamp_pos(r[10], L), s.end = clamp_pos(r[12], L);
    return s;
}

// 0..6
__device__ __forceinline__ int seg_of(const seg_row& s, int t) {
    const int c = (int)(s.s1 <= t) + (int)(s.s2 <= t) + (int)(s.s3 <= t) + (int)(s.s4 <= t) + (int)(s.s5 <= t);
    return t >= s.end ? 6 : c;
}

struct seg_w {
    float w[7];
};

__device__ __forceinline__ float pick(const seg_w& w, int k) {
    return k == 0 ? w.w[0] : k == 1 ? w.w[1] : k == 2 ? w.w[2] : k == 3 ? w.w[3] : k == 4 ? w.w[4] : k == 5 ? w.w[5] : w.w[6];
}

// grid (tiles, B): part[row * tiles + tile] = sum over the tile's positions of (double)w * (double)e, e as loss_partial forms it
__global__ __launch_bounds__(256) void seg_partial(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                   const float* __restrict__ noise, const int64_t* __restrict__ rois,
                                                   double* __restrict__ part, int L, int reg_l2, const seg_w w) {
    __shared__ double sm[4];
    const int row = blockIdx.y;
    const seg_row s = load_row(rois, row, L);
    const int t0 = blockIdx.x * TILE + (int)threadIdx.x * 4;
    double acc = 0.0;
    if (t0 < L) {                                        // L % 4 == 0: the four positions are inside the row or all outside
        const int64_t e0 = (int64_t)row * L + t0;
        const float4 xv = *reinterpret_cast<const float4*>(pred + e0);
        const float4 yv = *reinterpret_cast<const float4*>(tgt + e0);
        float x[4] = {xv.x, xv.y, xv.z, xv.w};
        const float y[4] = {yv.x, yv.y, yv.z, yv.w};
        if (noise) {
            const float4 zv = *reinterpret_cast<const float4*>(noise + e0);
            x[0] = x[0] + zv.x, x[1] = x[1] + zv.y, x[2] = x[2] + zv.z, x[3] = x[3] + zv.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = x[j] - y[j];
            const float e = reg_l2 ? d * d : fabsf(d);
            acc += (double)pick(w, seg_of(s, t0 + j)) * (double)e;
        }
    }
    acc = nef_block_sum_d(acc, sm);
    if (threadIdx.x == 0) part[(int64_t)row * gridDim.x + blockIdx.x] = acc;
}

// one block: partial i, i + 256, ... per thread, then the block sum -- the same order every time.  losses[1], losses[2] are loss_final's
__global__ __launch_bounds__(256) void seg_final(const double* __restrict__ part, float* __restrict__ losses, int64_t nparts, double n,
                                                 float f2) {
    __shared__ double sm[4];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = nef_block_sum_d(s, sm);
    if (threadIdx.x != 0) return;
    const float t3 = (float)(s / n) * f2;
    losses[3] = t3;
    losses[0] = (losses[1] + losses[2]) + t3;
}

// grid (tiles, B): g[i, t] = w[seg(i, t)] * g[i, t], one writer per element
__global__ __launch_bounds__(256) void seg_bwd_kernel(const int64_t* __restrict__ rois, float* __restrict__ g, int L, const seg_w w) {
    const int row = blockIdx.y;
    const int t0 = blockIdx.x * TILE + (int)threadIdx.x * 4;
    if (t0 >= L) return;
    const seg_row s = load_row(rois, row, L);
    float4* p = reinterpret_cast<float4*>(g + (int64_t)row * L + t0);
    const float4 v = *p;
    *p = make_float4(pick(w, seg_of(s, t0)) * v.x, pick(w, seg_of(s, t0 + 1)) * v.y, pick(w, seg_of(s, t0 + 2)) * v.z,
                     pick(w, seg_of(s, t0 + 3)) * v.w);
}

// one block per (sample, view) row: se[row, k] / cnt[row, k] = sum of ((double)x - (double)y)^2 / number of positions of segment k
__global__ __launch_bounds__(256) void view_seg_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                               const int64_t* __restrict__ rois, double* __restrict__ se,
                                                               int32_t* __restrict__ cnt, int Q, int L) {
    __shared__ double sm[4];
    const int row = blockIdx.x;
    const seg_row s = load_row(rois, row / Q, L);
    const float* x = pred + (int64_t)row * L;
    const float* y = gt + (int64_t)row * L;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0;
    for (int t0 = (int)threadIdx.x * 4; t0 < L; t0 += TILE) {
        const float4 xv = *reinterpret_cast<const float4*>(x + t0);
        const float4 yv = *reinterpret_cast<const float4*>(y + t0);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ys[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double d = (double)xs[j] - (double)ys[j];
            const double d2 = d * d;
            const int k = seg_of(s, t0 + j);
            a0 += k == 0 ? d2 : 0.0, c0 += k == 0;
            a1 += k == 1 ? d2 : 0.0, c1 += k == 1;
            a2 += k == 2 ? d2 : 0.0, c2 += k == 2;
            a3 += k == 3 ? d2 : 0.0, c3 += k == 3;
            a4 += k == 4 ? d2 : 0.0, c4 += k == 4;
            a5 += k == 5 ? d2 : 0.0, c5 += k == 5;
            a6 += k == 6 ? d2 : 0.0, c6 += k == 6;
        }
    }
    // counts go through the same fp64 block sum: integers below 2^53 add exactly
    a0 = nef_block_sum_d(a0, sm), a1 = nef_block_sum_d(a1, sm), a2 = nef_block_sum_d(a2, sm), a3 = nef_block_sum_d(a3, sm);
    a4 = nef_block_sum_d(a4, sm), a5 = nef_block_sum_d(a5, sm), a6 = nef_block_sum_d(a6, sm);
    const double n0 = nef_block_sum_d((double)c0, sm), n1 = nef_block_sum_d((double)c1, sm), n2 = nef_block_sum_d((double)c2, sm);
    const double n3 = nef_block_sum_d((double)c3, sm), n4 = nef_block_sum_d((double)c4, sm), n5 = nef_block_sum_d((double)c5, sm);
    const double n6 = nef_block_sum_d((double)c6, sm);
    if (threadIdx.x != 0) return;
    double* so = se + (int64_t)row * 7;
    int32_t* co = cnt + (int64_t)row * 7;
    so[0] = a0, so[1] = a1, so[2] = a2, so[3] = a3, so[4] = a4, so[5] = a5, so[6] = a6;
    co[0] = (int32_t)n0, co[1] = (int32_t)n1, co[2] = (int32_t)n2, co[3] = (int32_t)n3, co[4] = (int32_t)n4, co[5] = (int32_t)n5;
    co[6] = (int32_t)n6;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int seg_common(const nef_loss_seg_args* a, seg_w* w) {
    NEF_REQUIRE(a && a->rois, NEF_E_NULL);
    NEF_REQUIRE(a->B > 0 && a->L > 0 && a->B <= 65535 && a->L % 4 == 0, NEF_E_SHAPE);      // (B is a grid's y extent)
    for (int k = 0; k < 7; ++k) {
        NEF_REQUIRE(a->w[k] >= 0.f && a->w[k] <= 3.0e38f, NEF_E_SHAPE);                    // (NaN fails >=, inf fails <=)
        w->w[k] = a->w[k];
    }
    return NEF_OK;
}

}  // namespace

extern "C" {

size_t nef_loss_seg_args_bytes(void) { return sizeof(nef_loss_seg_args); }

size_t nef_loss_seg_ws_bytes(int B, int L) {
    if (B <= 0 || L <= 0) return 0;
    return (size_t)B * (size_t)nef_cdiv(L, TILE) * sizeof(double);
}

int nef_loss_seg_fwd(const nef_loss_seg_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->pred && a->target && a->losses, NEF_E_NULL);
    seg_w w;
    const int rc = seg_common(a, &w);
    if (rc != NEF_OK) return rc;
    NEF_REQUIRE(a->ws_bytes >= nef_loss_seg_ws_bytes(a->B, a->L), NEF_E_WORKSPACE);
    NEF_REQUIRE(a->ws, NEF_E_NULL);
    NEF_REQUIRE(aligned16(a->pred) && aligned16(a->target) && aligned16(a->noise) && ((uintptr_t)a->ws & 7) == 0, NEF_E_UNSUPPORTED);
    const int tiles = (int)nef_cdiv(a->L, TILE);
    hipLaunchKernelGGL(seg_partial, dim3(tiles, a->B), dim3(256), 0, (hipStream_t)stream, a->pred, a->target, a->noise, a->rois,
                       (double*)a->ws, a->L, a->reg_l2, w);
    hipLaunchKernelGGL(seg_final, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)a->ws, a->losses, (int64_t)a->B * tiles,
                       (double)a->B * (double)a->L, a->f2);
    return nef_launch_status();
}

int nef_loss_seg_bwd(const nef_loss_seg_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->g_pred, NEF_E_NULL);
    seg_w w;
    const int rc = seg_common(a, &w);
    if (rc != NEF_OK) return rc;
    NEF_REQUIRE(aligned16(a->g_pred), NEF_E_UNSUPPORTED);
    hipLaunchKernelGGL(seg_bwd_kernel, dim3((unsigned)nef_cdiv(a->L, TILE), a->B), dim3(256), 0, (hipStream_t)stream, a->rois, a->g_pred,
                       a->L, w);
    return nef_launch_status();
}

int nef_view_seg_metrics(const float* pred, const float* gt, const int64_t* rois, double* se, int32_t* cnt, int B, int Q, int L,
                         nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(pred && gt && rois && se && cnt, NEF_E_NULL);
    NEF_REQUIRE(B > 0 && Q > 0 && L > 0 && B <= 65535 && L % 4 == 0 && (int64_t)B * Q <= 0x7FFFFFFFll, NEF_E_SHAPE);
    NEF_REQUIRE(aligned16(pred) && aligned16(gt), NEF_E_UNSUPPORTED);
    hipLaunchKernelGGL(view_seg_metrics_kernel, dim3((unsigned)(B * Q)), dim3(256), 0, (hipStream_t)stream, pred, gt, rois, se, cnt, Q,
                       L);
    return nef_launch_status();
}

}  // extern "C"
