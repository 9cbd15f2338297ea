// The slope (first-difference) term of the training loss (cfg.SOLVER.slope_factor): factor * mean over rows of the row's mean
// |d| or d^2, d(i, t) = (x[t + 1] - x[t]) - (y[t + 1] - y[t]), forward and backward, and the test phase's squared slope error per
// (sample, view) row (cfg.SOLVER.slope_eval).  Definition, the row rule and the gradient: include/nefnet_hip.h (nef_loss_slope_args).
// Every difference is formed in fp64 from the fp32 values; every sum has a fixed order (no atomics).  All three kernels stage their
// stretch of x (+ noise) and y in LDS first -- 16-byte loads where the row's pointers are 16-byte aligned, scalar loads otherwise and for
// the halo -- so each element is read from memory once although two differences use it.
#include "nef_common.h"

namespace {

constexpr int TILE = NEF_LOSS_SLOPE_TILE;     // difference starts (forward, metrics) / positions (backward) per block
static_assert(TILE % 4 == 0, "the body of a tile is whole float4 groups");
constexpr int BODY = 4;                       // backward: the body sits at index 4 of the LDS rows, the left halo at 3
constexpr int NS = TILE + 8;

// xs / ys[k] = x (+ z) / y[lo + k] for k in [0, count): the caller guarantees lo + count <= L and 16-byte aligned xs, ys
__device__ __forceinline__ void stage(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int lo,
                                      int count, float* __restrict__ xs, float* __restrict__ ys) {
    const uintptr_t bits = (uintptr_t)(x + lo) | (uintptr_t)(y + lo) | (z ? (uintptr_t)(z + lo) : (uintptr_t)0);
    const int nv = (bits & 15) == 0 ? count >> 2 : 0;   // whole float4 groups
    const float4* x4 = reinterpret_cast<const float4*>(x + lo);
    const float4* y4 = reinterpret_cast<const float4*>(y + lo);
    for (int q = threadIdx.x; q < nv; q += 256) {
        float4 a = x4[q];
        if (z) {
            const float4 c = reinterpret_cast<const float4*>(z + lo)[q];
            a.x = a.x + c.x, a.y = a.y + c.y, a.z = a.z + c.z, a.w = a.w + c.w;
        }
        reinterpret_cast<float4*>(xs)[q] = a;
        reinterpret_cast<float4*>(ys)[q] = y4[q];
    }
    for (int k = nv * 4 + (int)threadIdx.x; k < count; k += 256) {
        xs[k] = z ? x[lo + k] + z[lo + k] : x[lo + k];
        ys[k] = y[lo + k];
    }
}

// d of the difference that starts at LDS index j
__device__ __forceinline__ double diff_at(const float* xs, const float* ys, int j) {
    return ((double)xs[j + 1] - (double)xs[j]) - ((double)ys[j + 1] - (double)ys[j]);
}

// grid (tiles, B): part[row * tiles + tile] = sum of e over the difference starts t of the tile, t in [0, end - 1) (0 when there is none)
__global__ __launch_bounds__(256) void slope_partial(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                     const float* __restrict__ noise, const int64_t* __restrict__ rois,
                                                     double* __restrict__ part, int L, int l2) {
    __shared__ double sm[4];
    __shared__ __attribute__((aligned(16))) float xs[NS], ys[NS];
    const int row = blockIdx.y;
    const int end = nef_row_end(rois, row, L);
    const int t0 = blockIdx.x * TILE;
    const int n = min(TILE, end - 1 - t0);               // difference starts of this tile: [t0, t0 + n)
    double acc = 0.0;
    if (n > 0) {                                         // block-uniform
        const int64_t r0 = (int64_t)row * L;
        stage(pred + r0, tgt + r0, noise ? noise + r0 : nullptr, t0, n + 1, xs, ys);      // t0 + n + 1 <= end <= L
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += 256) {
            const double d = diff_at(xs, ys, j);
            acc += l2 ? d * d : fabs(d);
        }
    }
    acc = nef_block_sum_d(acc, sm);
    if (threadIdx.x == 0) part[(int64_t)row * gridDim.x + blockIdx.x] = acc;
}

// one block: rows in the order r, r + 256, ... per thread, each row's tiles in order, then the block sum -- the same order every time
__global__ __launch_bounds__(256) void slope_final(const double* __restrict__ part, const int64_t* __restrict__ rois,
                                                   float* __restrict__ losses, int B, int L, int tiles, float factor, int slot) {
    __shared__ double sm[4];
    double s = 0.0, r = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        const int end = nef_row_end(rois, i, L);
        if (end < 2) continue;
        double si = 0.0;
        for (int t = 0; t < tiles; ++t) si += part[(int64_t)i * tiles + t];
        s += si / (double)(end - 1);
        r += 1.0;
    }
    s = nef_block_sum_d(s, sm);
    r = nef_block_sum_d(r, sm);
    if (threadIdx.x != 0) return;
    const double term = r > 0.0 ? (double)factor * (s / r) : 0.0;
    const float ts = (float)term;
    losses[slot] = ts;
    losses[0] = losses[0] + ts;
}

// grid (tiles, B), 256 threads: the block owns positions [t0, t0 + TILE) of its row below the row's end.  x and y of
// [t0 - 1, t0 + TILE + 1) are staged in LDS (body at index BODY, so its float4 stores stay aligned); position t adds
// scale * (s(t - 1) - s(t)), s = 0 for a difference that does not exist.
__global__ __launch_bounds__(256) void slope_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                        const float* __restrict__ noise, const int64_t* __restrict__ rois,
                                                        const float* __restrict__ gscale, float* __restrict__ g_pred, int B, int L,
                                                        float factor, int l2) {
    __shared__ double sm[4];
    __shared__ __attribute__((aligned(16))) float xs[NS], ys[NS];
    const int row = blockIdx.y;
    const int end = nef_row_end(rois, row, L);
    const int t0 = blockIdx.x * TILE;
    if (end < 2 || t0 >= end) return;                    // block-uniform: a row without a difference, a tile behind the row's end
    double r = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) r += nef_row_end(rois, i, L) >= 2 ? 1.0 : 0.0;
    r = nef_block_sum_d(r, sm);                          // >= 1: this row counts
    const int64_t r0 = (int64_t)row * L;
    const float* x = pred + r0;
    const float* y = tgt + r0;
    const float* z = noise ? noise + r0 : nullptr;
    const int t1 = min(t0 + TILE, end);                  // positions of this block: [t0, t1)
    const int t2 = min(t1 + 1, end);                     // ... and the right halo, when the row goes on
    stage(x, y, z, t0, t2 - t0, xs + BODY, ys + BODY);
    if (threadIdx.x == 0 && t0 > 0) {
        xs[BODY - 1] = z ? x[t0 - 1] + z[t0 - 1] : x[t0 - 1];
        ys[BODY - 1] = y[t0 - 1];
    }
    __syncthreads();
    const double gs = gscale ? (double)gscale[0] : 1.0;
    const double scale = (double)factor * gs / (r * (double)(end - 1));
    for (int t = t0 + threadIdx.x; t < t1; t += 256) {
        const int j = BODY + (t - t0);
        double sl = 0.0, sr = 0.0;                       // s(t - 1), s(t)
        if (t > 0) {
            const double d = diff_at(xs, ys, j - 1);
            sl = l2 ? 2.0 * d : (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0));
        }
        if (t < end - 1) {
            const double d = diff_at(xs, ys, j);
            sr = l2 ? 2.0 * d : (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0));
        }
        g_pred[r0 + t] += (float)(scale * (sl - sr));
    }
}

// one block per (sample, view) row: se[row] = sum of d^2 over the row's differences, tile by tile in order; cnt[row] = their number
__global__ __launch_bounds__(256) void view_slope_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                 const int64_t* __restrict__ rois, double* __restrict__ se,
                                                                 int32_t* __restrict__ cnt, int Q, int L) {
    __shared__ double sm[4];
    __shared__ __attribute__((aligned(16))) float xs[NS], ys[NS];
    const int row = blockIdx.x;
    const int end = nef_row_end(rois, row / Q, L);
    const int64_t r0 = (int64_t)row * L;
    double acc = 0.0;
    for (int t0 = 0; t0 < end - 1; t0 += TILE) {         // block-uniform
        const int n = min(TILE, end - 1 - t0);
        __syncthreads();                                 // the previous tile has been read
        stage(pred + r0, gt + r0, nullptr, t0, n + 1, xs, ys);
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += 256) {
            const double d = diff_at(xs, ys, j);
            acc += d * d;
        }
    }
    acc = nef_block_sum_d(acc, sm);
    if (threadIdx.x == 0) {
        se[row] = acc;
        cnt[row] = end > 1 ? end - 1 : 0;
    }
}

int slope_common(const nef_loss_slope_args* a) {
    NEF_REQUIRE(a && a->pred && a->target, NEF_E_NULL);
    NEF_REQUIRE(a->B > 0 && a->L > 0 && a->B <= 65535 && a->factor >= 0.f, NEF_E_SHAPE);       // (B is a grid's y extent; NaN fails >=)
    return NEF_OK;
}

}  // namespace

extern "C" {

size_t nef_loss_slope_args_bytes(void) { return sizeof(nef_loss_slope_args); }

size_t nef_loss_slope_ws_bytes(int B, int L) {
    if (B <= 0 || L <= 0) return 0;
    return (size_t)B * (size_t)nef_cdiv(L, TILE) * sizeof(double);
}

int nef_loss_slope_fwd(const nef_loss_slope_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->losses, NEF_E_NULL);
    const int rc = slope_common(a);
    if (rc != NEF_OK) return rc;
    NEF_REQUIRE(a->slot == 4 || a->slot == 5, NEF_E_SHAPE);
    NEF_REQUIRE(a->ws_bytes >= nef_loss_slope_ws_bytes(a->B, a->L), NEF_E_WORKSPACE);
    NEF_REQUIRE(a->ws, NEF_E_NULL);
    const int tiles = (int)nef_cdiv(a->L, TILE);
    hipLaunchKernelGGL(slope_partial, dim3(tiles, a->B), dim3(256), 0, (hipStream_t)stream, a->pred, a->target, a->noise, a->rois,
                       (double*)a->ws, a->L, a->l2);
    hipLaunchKernelGGL(slope_final, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)a->ws, a->rois, a->losses, a->B, a->L,
                       tiles, a->factor, a->slot);
    return nef_launch_status();
}

int nef_loss_slope_bwd(const nef_loss_slope_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->g_pred, NEF_E_NULL);
    const int rc = slope_common(a);
    if (rc != NEF_OK) return rc;
    hipLaunchKernelGGL(slope_bwd_kernel, dim3((unsigned)nef_cdiv(a->L, TILE), a->B), dim3(256), 0, (hipStream_t)stream, a->pred,
                       a->target, a->noise, a->rois, a->gscale, a->g_pred, a->B, a->L, a->factor, a->l2);
    return nef_launch_status();
}

int nef_view_slope_metrics(const float* pred, const float* gt, const int64_t* rois, double* se, int32_t* cnt, int B, int Q, int L,
                           nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(pred && gt && se && cnt, NEF_E_NULL);
    NEF_REQUIRE(B > 0 && Q > 0 && L > 0 && (int64_t)B * Q <= 0x7FFFFFFFll, NEF_E_SHAPE);
    hipLaunchKernelGGL(view_slope_metrics_kernel, dim3((unsigned)(B * Q)), dim3(256), 0, (hipStream_t)stream, pred, gt, rois, se, cnt,
                       Q, L);
    return nef_launch_status();
}

}  // extern "C"
