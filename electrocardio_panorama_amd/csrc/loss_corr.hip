// The correlation term of the training loss (cfg.SOLVER.corr_factor): factor * mean over rows of 1 - r_i, r_i the Pearson correlation
// coefficient of the row's prediction (+ noise) and target, forward and backward, and the test phase's moments per (sample, view) row
// (cfg.SOLVER.corr_eval).  Definition, the row rule and the gradient: include/nefnet_hip.h (nef_loss_corr_args).
// Every element's gradient depends on moments of its whole row, so the backward is reduce-then-apply: the partial-sum launch of the
// forward, a one-block finish that leaves four numbers per row, and an apply launch.  Everything is fp64 from the fp32 values; every sum
// has a fixed order (no atomics).  Each element is used once, so nothing is staged in LDS: 16-byte loads where the tile's pointers are
// 16-byte aligned, scalar loads otherwise.
#include "nef_common.h"

// no fused multiply-adds: pred == target has to give the SAME bits for sum u^2, sum w^2 and sum u w, whatever the compiler would fuse
#pragma clang fp contract(off)

namespace {

constexpr int TILE = NEF_LOSS_CORR_TILE;      // positions per block of the partial-sum and apply launches
static_assert(TILE % 4 == 0, "a tile is whole float4 groups");
constexpr int NSUM = 5;                       // sum u, sum w, sum u^2, sum w^2, sum u w
constexpr int NSTAT = 4;                      // mu, mw, a, k per row

__device__ __forceinline__ void add_sample(double (&s)[NSUM], float xf, float yf, double x0, double y0) {
    const double u = (double)xf - x0, w = (double)yf - y0;
    s[0] += u;
    s[1] += w;
    s[2] += u * u;
    s[3] += w * w;
    s[4] += u * w;
}

// s += the five shifted sums over x (+ z) / y[lo + k], k in [0, count): the caller guarantees lo + count <= L
__device__ __forceinline__ void tile_sums(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int lo,
                                          int count, double x0, double y0, double (&s)[NSUM]) {
    const uintptr_t bits = (uintptr_t)(x + lo) | (uintptr_t)(y + lo) | (z ? (uintptr_t)(z + lo) : (uintptr_t)0);
    const bool vec = (bits & 15) == 0;
    const int nv = count >> 2;                          // whole groups of four: a thread owns the same samples, in the same order, on both
                                                        // paths, so the sums do not depend on the alignment
    for (int q = threadIdx.x; q < nv; q += 256) {
        const int k = lo + 4 * q;
        float4 a, b;
        if (vec) {
            a = *reinterpret_cast<const float4*>(x + k);
            b = *reinterpret_cast<const float4*>(y + k);
        } else {
            a = make_float4(x[k], x[k + 1], x[k + 2], x[k + 3]);
            b = make_float4(y[k], y[k + 1], y[k + 2], y[k + 3]);
        }
        if (z) {
            const float4 c = vec ? *reinterpret_cast<const float4*>(z + k) : make_float4(z[k], z[k + 1], z[k + 2], z[k + 3]);
            a.x = a.x + c.x, a.y = a.y + c.y, a.z = a.z + c.z, a.w = a.w + c.w;
        }
        add_sample(s, a.x, b.x, x0, y0);
        add_sample(s, a.y, b.y, x0, y0);
        add_sample(s, a.z, b.z, x0, y0);
        add_sample(s, a.w, b.w, x0, y0);
    }
    for (int k = nv * 4 + (int)threadIdx.x; k < count; k += 256)
        add_sample(s, z ? x[lo + k] + z[lo + k] : x[lo + k], y[lo + k], x0, y0);
}

__device__ __forceinline__ void block_sum5(double (&s)[NSUM], double (*sm)[4]) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) s[k] = nef_wave_sum_d(s[k]);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) sm[k][w] = s[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NSUM; ++k) s[k] = sm[k][0] + sm[k][1] + sm[k][2] + sm[k][3];
}

// grid (tiles, B): part[(row * tiles + tile) * 5 ..] = the five sums over the tile's positions below the row's end (0 when there is none),
// on values shifted by the row's first sample
__global__ __launch_bounds__(256) void corr_partial(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                    const float* __restrict__ noise, const int64_t* __restrict__ rois,
                                                    double* __restrict__ part, int L) {
    __shared__ double sm[NSUM][4];
    const int row = blockIdx.y;
    const int end = nef_row_end(rois, row, L);
    const int t0 = blockIdx.x * TILE;
    const int n = min(TILE, end - t0);                   // positions of this tile: [t0, t0 + n)
    double s[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (n > 0) {                                         // block-uniform; end >= 1, so the row has a first sample
        const int64_t r0 = (int64_t)row * L;
        const float* x = pred + r0;
        const float* y = tgt + r0;
        const float* z = noise ? noise + r0 : nullptr;
        tile_sums(x, y, z, t0, n, (double)(z ? x[0] + z[0] : x[0]), (double)y[0], s);
    }
    block_sum5(s, sm);
    if (threadIdx.x == 0) {
        double* o = part + ((int64_t)row * gridDim.x + blockIdx.x) * NSUM;
#pragma unroll
        for (int k = 0; k < NSUM; ++k) o[k] = s[k];
    }
}

// the moments of row i from its tiles' partial sums, in tile order; n >= 2
struct RowMoments {
    double mu, mw, vx, vy, c;
};

__device__ __forceinline__ RowMoments row_moments(const double* __restrict__ part, int i, int tiles, int n) {
    double s[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < tiles; ++t) {
        const double* p = part + ((int64_t)i * tiles + t) * NSUM;
#pragma unroll
        for (int k = 0; k < NSUM; ++k) s[k] += p[k];
    }
    const double dn = (double)n;
    RowMoments m;
    m.mu = s[0] / dn;
    m.mw = s[1] / dn;
    m.vx = s[2] / dn - m.mu * m.mu;
    m.vy = s[3] / dn - m.mw * m.mw;
    m.c = s[4] / dn - m.mu * m.mw;
    return m;
}

// one block: rows in the order r, r + 256, ... per thread, each row's tiles in order, then the block sum -- the same order every time
__global__ __launch_bounds__(256) void corr_final(const double* __restrict__ part, const int64_t* __restrict__ rois,
                                                  float* __restrict__ losses, int B, int L, int tiles, float factor, double eps, int slot) {
    __shared__ double sm[4];
    double s = 0.0, r = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        const int end = nef_row_end(rois, i, L);
        if (end < 2) continue;
        const RowMoments m = row_moments(part, i, tiles, end);
        const double D = sqrt((m.vx + eps) * (m.vy + eps));
        s += 1.0 - (m.c + eps) / D;
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

// one block: stat[i * 4 ..] = mu, mw, a = -factor / (R n D), k = r D / (vx + eps) of row i; zeros for a row that does not count
__global__ __launch_bounds__(256) void corr_bwd_final(const double* __restrict__ part, const int64_t* __restrict__ rois,
                                                      double* __restrict__ stat, int B, int L, int tiles, float factor, double eps) {
    __shared__ double sm[4];
    double R = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) R += nef_row_end(rois, i, L) >= 2 ? 1.0 : 0.0;
    R = nef_block_sum_d(R, sm);
    for (int i = threadIdx.x; i < B; i += 256) {
        const int end = nef_row_end(rois, i, L);
        double* o = stat + (int64_t)i * NSTAT;
        if (end < 2) {
            o[0] = 0.0, o[1] = 0.0, o[2] = 0.0, o[3] = 0.0;
            continue;
        }
        const RowMoments m = row_moments(part, i, tiles, end);
        const double D = sqrt((m.vx + eps) * (m.vy + eps));
        const double r = (m.c + eps) / D;
        o[0] = m.mu;
        o[1] = m.mw;
        o[2] = -(double)factor / (R * (double)end * D);
        o[3] = r * D / (m.vx + eps);
    }
}

__device__ __forceinline__ float grad_at(float g, float xf, float yf, double x0, double y0, double mu, double mw, double ga, double k) {
    const double u = (double)xf - x0, w = (double)yf - y0;
    return g + (float)(ga * ((w - mw) - k * (u - mu)));
}

// grid (tiles, B), 256 threads: the block owns positions [t0, t0 + TILE) of its row below the row's end; one writer per element
__global__ __launch_bounds__(256) void corr_apply(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                  const float* __restrict__ noise, const int64_t* __restrict__ rois,
                                                  const float* __restrict__ gscale, const double* __restrict__ stat,
                                                  float* __restrict__ g_pred, int L) {
    const int row = blockIdx.y;
    const int end = nef_row_end(rois, row, L);
    const int t0 = blockIdx.x * TILE;
    if (end < 2 || t0 >= end) return;                    // block-uniform: a row that does not count, a tile behind the row's end
    const int64_t r0 = (int64_t)row * L;
    const float* x = pred + r0;
    const float* y = tgt + r0;
    const float* z = noise ? noise + r0 : nullptr;
    float* g = g_pred + r0;
    const double x0 = (double)(z ? x[0] + z[0] : x[0]), y0 = (double)y[0];
    const double* st = stat + (int64_t)row * NSTAT;
    const double mu = st[0], mw = st[1], k = st[3];
    const double ga = (gscale ? (double)gscale[0] : 1.0) * st[2];
    const int count = min(TILE, end - t0);               // positions of this block: [t0, t0 + count), t0 + count <= end <= L
    const uintptr_t bits = (uintptr_t)(x + t0) | (uintptr_t)(y + t0) | (uintptr_t)(g + t0) | (z ? (uintptr_t)(z + t0) : (uintptr_t)0);
    const int nv = (bits & 15) == 0 ? count >> 2 : 0;    // whole float4 groups
    for (int q = threadIdx.x; q < nv; q += 256) {
        float4 a = reinterpret_cast<const float4*>(x + t0)[q];
        if (z) {
            const float4 c = reinterpret_cast<const float4*>(z + t0)[q];
            a.x = a.x + c.x, a.y = a.y + c.y, a.z = a.z + c.z, a.w = a.w + c.w;
        }
        const float4 b = reinterpret_cast<const float4*>(y + t0)[q];
        float4 o = reinterpret_cast<float4*>(g + t0)[q];
        o.x = grad_at(o.x, a.x, b.x, x0, y0, mu, mw, ga, k);
        o.y = grad_at(o.y, a.y, b.y, x0, y0, mu, mw, ga, k);
        o.z = grad_at(o.z, a.z, b.z, x0, y0, mu, mw, ga, k);
        o.w = grad_at(o.w, a.w, b.w, x0, y0, mu, mw, ga, k);
        reinterpret_cast<float4*>(g + t0)[q] = o;
    }
    for (int j = nv * 4 + (int)threadIdx.x; j < count; j += 256) {
        const int t = t0 + j;
        g[t] = grad_at(g[t], z ? x[t] + z[t] : x[t], y[t], x0, y0, mu, mw, ga, k);
    }
}

// one block per (sample, view) row: mom[row * 3 ..] = vx, vy, c over [0, end), tile by tile in order; cnt[row] = end
__global__ __launch_bounds__(256) void view_corr_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                const int64_t* __restrict__ rois, double* __restrict__ mom,
                                                                int32_t* __restrict__ cnt, int Q, int L) {
    __shared__ double sm[NSUM][4];
    const int row = blockIdx.x;
    const int end = nef_row_end(rois, row / Q, L);
    const int64_t r0 = (int64_t)row * L;
    double s[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (end > 0) {                                       // block-uniform
        const double x0 = (double)pred[r0], y0 = (double)gt[r0];
        for (int t0 = 0; t0 < end; t0 += TILE) tile_sums(pred + r0, gt + r0, nullptr, t0, min(TILE, end - t0), x0, y0, s);
    }
    block_sum5(s, sm);
    if (threadIdx.x != 0) return;
    double vx = 0.0, vy = 0.0, c = 0.0;
    if (end > 0) {
        const double dn = (double)end, mu = s[0] / dn, mw = s[1] / dn;
        vx = s[2] / dn - mu * mu;
        vy = s[3] / dn - mw * mw;
        c = s[4] / dn - mu * mw;
    }
    mom[(int64_t)row * 3 + 0] = vx;
    mom[(int64_t)row * 3 + 1] = vy;
    mom[(int64_t)row * 3 + 2] = c;
    cnt[row] = end;
}

int corr_common(const nef_loss_corr_args* a) {
    NEF_REQUIRE(a && a->pred && a->target, NEF_E_NULL);
    // (B is a grid's y extent; NaN fails >=)
    NEF_REQUIRE(a->B > 0 && a->L > 0 && a->B <= 65535 && a->factor >= 0.f && a->eps >= 0.0, NEF_E_SHAPE);
    return NEF_OK;
}

}  // namespace

extern "C" {

size_t nef_loss_corr_args_bytes(void) { return sizeof(nef_loss_corr_args); }

size_t nef_loss_corr_ws_bytes(int B, int L) {
    if (B <= 0 || L <= 0) return 0;
    return (size_t)B * ((size_t)nef_cdiv(L, TILE) * NSUM + NSTAT) * sizeof(double);
}

int nef_loss_corr_fwd(const nef_loss_corr_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->losses, NEF_E_NULL);
    const int rc = corr_common(a);
    if (rc != NEF_OK) return rc;
    NEF_REQUIRE(a->slot >= 4 && a->slot <= 6, NEF_E_SHAPE);
    NEF_REQUIRE(a->ws_bytes >= nef_loss_corr_ws_bytes(a->B, a->L), NEF_E_WORKSPACE);
    NEF_REQUIRE(a->ws, NEF_E_NULL);
    const int tiles = (int)nef_cdiv(a->L, TILE);
    hipLaunchKernelGGL(corr_partial, dim3(tiles, a->B), dim3(256), 0, (hipStream_t)stream, a->pred, a->target, a->noise, a->rois,
                       (double*)a->ws, a->L);
    hipLaunchKernelGGL(corr_final, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)a->ws, a->rois, a->losses, a->B, a->L,
                       tiles, a->factor, a->eps, a->slot);
    return nef_launch_status();
}

int nef_loss_corr_bwd(const nef_loss_corr_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->g_pred, NEF_E_NULL);
    const int rc = corr_common(a);
    if (rc != NEF_OK) return rc;
    NEF_REQUIRE(a->ws_bytes >= nef_loss_corr_ws_bytes(a->B, a->L), NEF_E_WORKSPACE);
    NEF_REQUIRE(a->ws, NEF_E_NULL);
    const int tiles = (int)nef_cdiv(a->L, TILE);
    double* part = (double*)a->ws;
    double* stat = part + (size_t)a->B * tiles * NSUM;
    hipLaunchKernelGGL(corr_partial, dim3(tiles, a->B), dim3(256), 0, (hipStream_t)stream, a->pred, a->target, a->noise, a->rois, part,
                       a->L);
    hipLaunchKernelGGL(corr_bwd_final, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)part, a->rois, stat, a->B, a->L, tiles,
                       a->factor, a->eps);
    hipLaunchKernelGGL(corr_apply, dim3(tiles, a->B), dim3(256), 0, (hipStream_t)stream, a->pred, a->target, a->noise, a->rois, a->gscale,
                       (const double*)stat, a->g_pred, a->L);
    return nef_launch_status();
}

int nef_view_corr_metrics(const float* pred, const float* gt, const int64_t* rois, double* mom, int32_t* cnt, int B, int Q, int L,
                          nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(pred && gt && mom && cnt, NEF_E_NULL);
    NEF_REQUIRE(B > 0 && Q > 0 && L > 0 && (int64_t)B * Q <= 0x7FFFFFFFll, NEF_E_SHAPE);
    hipLaunchKernelGGL(view_corr_metrics_kernel, dim3((unsigned)(B * Q)), dim3(256), 0, (hipStream_t)stream, pred, gt, rois, mom, cnt,
                       Q, L);
    return nef_launch_status();
}

}  // extern "C"
