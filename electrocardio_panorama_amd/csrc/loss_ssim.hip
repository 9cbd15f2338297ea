// The structural-similarity term of the training loss (cfg.SOLVER.ssim_factor): factor * (1 - mean SSIM), forward and backward, with the
// SSIM of view_metrics_kernel (metrics.hip; utils/metric.py:ssim_1d) -- 7-tap uniform window, sample covariance (7/6), c1 = 1e-4,
// c2 = 9e-4, full windows only -- so that 1 - term / factor is what the test phase reports on the same rows.  Definition, the row rule
// and the gradient: include/nefnet_hip.h (nef_loss_ssim_args).  All window arithmetic is fp64, as in view_metrics_kernel: ~60 fp64
// operations per element, nothing beside the step; every sum has a fixed order (no atomics).
#include "nef_common.h"

namespace {

constexpr int WIN = 7;
constexpr int TILE = NEF_LOSS_SSIM_TILE;      // window starts (forward) / positions (backward) per block
constexpr int HALO = WIN - 1;
constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03, COV_NORM = (double)WIN / (WIN - 1.0);

// the five window moments -> means and (co)variances
struct ssim_win {
    double ux, uy, vx, vy, vxy;
};
__device__ __forceinline__ ssim_win win_stats(double sx, double sy, double sxx, double syy, double sxy) {
    ssim_win w;
    w.ux = sx / WIN, w.uy = sy / WIN;
    w.vx = COV_NORM * (sxx / WIN - w.ux * w.ux);
    w.vy = COV_NORM * (syy / WIN - w.uy * w.uy);
    w.vxy = COV_NORM * (sxy / WIN - w.ux * w.uy);
    return w;
}

// grid (tiles, B): part[row * tiles + tile] = sum of S_p over the window starts p of the tile, p in [0, end - 6) (0 when there is none)
__global__ __launch_bounds__(256) void ssim_partial(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                    const float* __restrict__ noise, const int64_t* __restrict__ rois,
                                                    double* __restrict__ part, int L) {
    __shared__ double sm[4];
    const int row = blockIdx.y;
    const int end = nef_row_end(rois, row, L);
    const int p0 = blockIdx.x * TILE;
    const int p1 = min(p0 + TILE, end - HALO);           // window starts of this tile: [p0, p1)
    const float* x = pred + (int64_t)row * L;
    const float* y = tgt + (int64_t)row * L;
    const float* z = noise ? noise + (int64_t)row * L : nullptr;
    double ss = 0.0;
    for (int p = p0 + threadIdx.x; p < p1; p += 256) {
        double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const double a = (double)(z ? x[p + k] + z[p + k] : x[p + k]), b = (double)y[p + k];
            sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
        }
        const ssim_win w = win_stats(sx, sy, sxx, syy, sxy);
        ss += ((2 * w.ux * w.uy + C1) * (2 * w.vxy + C2)) / ((w.ux * w.ux + w.uy * w.uy + C1) * (w.vx + w.vy + C2));
    }
    ss = nef_block_sum_d(ss, sm);
    if (threadIdx.x == 0) part[(int64_t)row * gridDim.x + blockIdx.x] = ss;
}

// one block: rows in the order r, r + 256, ... per thread, each row's tiles in order, then the block sum -- the same order every time
__global__ __launch_bounds__(256) void ssim_final(const double* __restrict__ part, const int64_t* __restrict__ rois,
                                                  float* __restrict__ losses, int B, int L, int tiles, float factor) {
    __shared__ double sm[4];
    double s = 0.0, r = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        const int end = nef_row_end(rois, i, L);
        if (end < WIN) continue;
        double si = 0.0;
        for (int t = 0; t < tiles; ++t) si += part[(int64_t)i * tiles + t];
        s += si / (double)(end - HALO);
        r += 1.0;
    }
    s = nef_block_sum_d(s, sm);
    r = nef_block_sum_d(r, sm);
    if (threadIdx.x != 0) return;
    const double term = r > 0.0 ? (double)factor * (1.0 - s / r) : 0.0;
    const float t4 = (float)term;
    losses[4] = t4;
    losses[0] = losses[0] + t4;
}

// grid (tiles, B), 256 threads: the block owns positions [t0, t0 + TILE) of its row.  The windows that hold one of them start in
// [t0 - 6, t0 + TILE): x and y of [t0 - 6, t0 + TILE + 6) are staged in LDS, every window's (a_p, b_p, c_p) -- dS_p/dx_t =
// a_p + b_p x_t + c_p y_t for t inside the window -- is formed once in fp64 into LDS (zeros for a window that does not exist), and each
// position adds its <= 7 windows.
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                       const float* __restrict__ noise, const int64_t* __restrict__ rois,
                                                       const float* __restrict__ gscale, float* __restrict__ g_pred, int B, int L,
                                                       float factor) {
    constexpr int NX = TILE + 2 * HALO, NW = TILE + HALO;
    __shared__ double sm[4];
    __shared__ float xs[NX], ys[NX];
    __shared__ double ca[NW], cb[NW], cc[NW];
    const int row = blockIdx.y;
    const int end = nef_row_end(rois, row, L);
    const int t0 = blockIdx.x * TILE;
    if (end < WIN || t0 >= end) return;                  // block-uniform: a row without a window, a tile behind the row's end
    double r = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) r += nef_row_end(rois, i, L) >= WIN ? 1.0 : 0.0;
    r = nef_block_sum_d(r, sm);                          // >= 1: this row counts
    const float* x = pred + (int64_t)row * L;
    const float* y = tgt + (int64_t)row * L;
    const float* z = noise ? noise + (int64_t)row * L : nullptr;
    for (int j = threadIdx.x; j < NX; j += 256) {
        const int t = t0 - HALO + j;
        const bool in = t >= 0 && t < end;
        xs[j] = in ? (z ? x[t] + z[t] : x[t]) : 0.f;
        ys[j] = in ? y[t] : 0.f;
    }
    __syncthreads();
    for (int w = threadIdx.x; w < NW; w += 256) {
        const int p = t0 - HALO + w;                     // the window [p, p + 7) = xs[w .. w + 6]
        double a = 0.0, b = 0.0, c = 0.0;
        if (p >= 0 && p + WIN <= end) {
            double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const double u = (double)xs[w + k], v = (double)ys[w + k];
                sx += u; sy += v; sxx += u * u; syy += v * v; sxy += u * v;
            }
            const ssim_win s = win_stats(sx, sy, sxx, syy, sxy);
            const double A1 = 2 * s.ux * s.uy + C1, A2 = 2 * s.vxy + C2;
            const double B1 = s.ux * s.ux + s.uy * s.uy + C1, B2 = s.vx + s.vy + C2;
            const double S = (A1 * A2) / (B1 * B2);
            const double d_ux = 2.0 * (s.uy * A2 - s.ux * S * B2) / (B1 * B2);
            const double d_vx = -S / B2;
            const double d_vxy = 2.0 * A1 / (B1 * B2);
            b = 2.0 * COV_NORM * d_vx / WIN;
            c = COV_NORM * d_vxy / WIN;
            a = d_ux / WIN - b * s.ux - c * s.uy;
        }
        ca[w] = a, cb[w] = b, cc[w] = c;
    }
    __syncthreads();
    const double gs = gscale ? (double)gscale[0] : 1.0;
    const double scale = -(double)factor * gs / (r * (double)(end - HALO));
    const int t1 = min(t0 + TILE, end);
    for (int t = t0 + threadIdx.x; t < t1; t += 256) {
        const int j = t - t0;                            // windows t - 6 .. t = ca[j .. j + 6]; the position is xs[j + 6]
        const double u = (double)xs[j + HALO], v = (double)ys[j + HALO];
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < WIN; ++k) acc += ca[j + k] + cb[j + k] * u + cc[j + k] * v;
        g_pred[(int64_t)row * L + t] += (float)(scale * acc);
    }
}

}  // namespace

extern "C" {

size_t nef_loss_ssim_args_bytes(void) { return sizeof(nef_loss_ssim_args); }

size_t nef_loss_ssim_ws_bytes(int B, int L) {
    if (B <= 0 || L <= 0) return 0;
    return (size_t)B * (size_t)nef_cdiv(L, NEF_LOSS_SSIM_TILE) * sizeof(double);
}

static int ssim_common(const nef_loss_ssim_args* a) {
    NEF_REQUIRE(a && a->pred && a->target, NEF_E_NULL);
    NEF_REQUIRE(a->B > 0 && a->L > 0 && a->B <= 65535 && a->factor >= 0.f, NEF_E_SHAPE);       // (B is a grid's y extent; NaN fails >=)
    return NEF_OK;
}

int nef_loss_ssim_fwd(const nef_loss_ssim_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->losses, NEF_E_NULL);
    const int rc = ssim_common(a);
    if (rc != NEF_OK) return rc;
    NEF_REQUIRE(a->ws_bytes >= nef_loss_ssim_ws_bytes(a->B, a->L), NEF_E_WORKSPACE);
    NEF_REQUIRE(a->ws, NEF_E_NULL);
    const int tiles = (int)nef_cdiv(a->L, TILE);
    hipLaunchKernelGGL(ssim_partial, dim3(tiles, a->B), dim3(256), 0, (hipStream_t)stream, a->pred, a->target, a->noise, a->rois,
                       (double*)a->ws, a->L);
    hipLaunchKernelGGL(ssim_final, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)a->ws, a->rois, a->losses, a->B, a->L,
                       tiles, a->factor);
    return nef_launch_status();
}

int nef_loss_ssim_bwd(const nef_loss_ssim_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->g_pred, NEF_E_NULL);
    const int rc = ssim_common(a);
    if (rc != NEF_OK) return rc;
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3((unsigned)nef_cdiv(a->L, TILE), a->B), dim3(256), 0, (hipStream_t)stream, a->pred,
                       a->target, a->noise, a->rois, a->gscale, a->g_pred, a->B, a->L, a->factor);
    return nef_launch_status();
}

}  // extern "C"
