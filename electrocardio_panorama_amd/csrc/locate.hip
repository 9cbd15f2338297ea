// Locating a lead's viewing angle by a scored panorama search (Model_nefnet.locate, engine.locate): the score of every (sample, candidate
// angle) view against the sample's observed rows, the deterministic arg-best and the next level's candidates.  Definitions and the
// argument rules: include/nefnet_hip.h (nef_locate_score_args).
// The scorer is one wave per view row: the row stays in the wave's registers while the wave walks the R observed rows, so the views -- the
// only large operand -- are read from HBM once; the observed rows are B * R * L floats and hit L2.  Everything is fp64 from the fp32
// values, every sum has a fixed order (no atomics, no LDS: the four waves of a block never talk to each other), 16-byte loads where a
// row's pointer is 16-byte aligned and scalar loads otherwise, in the same order of additions.
#include <math.h>

#include "nef_common.h"

// no fused multiply-adds: p == y has to give the SAME bits for sum u^2, sum w^2 and sum u w (r == 1.0, score 0.0 exactly), and the
// candidates are one rounded multiply and one rounded add
#pragma clang fp contract(off)

namespace {

constexpr int SEG = NEF_LOCATE_SEG;           // positions of a row that a wave holds in registers
constexpr int NV = SEG / (NEF_WAVE * 4);      // float4 groups per lane and segment
static_assert(NV * NEF_WAVE * 4 == SEG && NV >= 1, "a segment is whole float4 groups for every lane");
constexpr int NSUM = 5;                       // mode 1: sum u, sum w, sum u^2, sum w^2, sum u w; mode 0: sum d^2 in slot 0

struct Seg {
    float v[NV][4];
};

// lane `lane`'s share of positions [k0, min(k0 + SEG, n)) of row x: group j holds positions k0 + (j * 64 + lane) * 4 + (0 .. 3); positions
// at and behind n are never read (zeros stand in and are not summed)
__device__ __forceinline__ Seg load_seg(const float* __restrict__ x, int k0, int n, int lane, bool vec) {
    Seg s;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int k = k0 + (j * NEF_WAVE + lane) * 4;
        const int c = n - k;                              // positions of this group inside the row
        if (c >= 4) {
            float4 q;
            if (vec) q = *reinterpret_cast<const float4*>(x + k);
            else q = make_float4(x[k], x[k + 1], x[k + 2], x[k + 3]);
            s.v[j][0] = q.x, s.v[j][1] = q.y, s.v[j][2] = q.z, s.v[j][3] = q.w;
        } else {                                          // the row's last, partial group (or nothing): one by one on both paths
            s.v[j][0] = c > 0 ? x[k] : 0.f;
            s.v[j][1] = c > 1 ? x[k + 1] : 0.f;
            s.v[j][2] = c > 2 ? x[k + 2] : 0.f;
            s.v[j][3] = 0.f;
        }
    }
    return s;
}

template <int MODE>
__device__ __forceinline__ void add_sample(double (&s)[NSUM], float pf, float yf, double p0, double y0) {
    if (MODE == 0) {
        const double d = (double)pf - (double)yf;
        s[0] += d * d;
    } else {
        const double u = (double)pf - p0, w = (double)yf - y0;
        s[0] += u;
        s[1] += w;
        s[2] += u * u;
        s[3] += w * w;
        s[4] += u * w;
    }
}

// the lane's positions of one segment, in rising order
template <int MODE>
__device__ __forceinline__ void add_seg(double (&s)[NSUM], const Seg& p, const Seg& y, int k0, int n, int lane, double p0, double y0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = n - (k0 + (j * NEF_WAVE + lane) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c > e) add_sample<MODE>(s, p.v[j][e], y.v[j][e], p0, y0);
    }
}

// every lane gets the score of the row from the lanes' sums; n >= 1 (mode 0) / n >= 2 (mode 1)
template <int MODE>
__device__ __forceinline__ double finish(double (&s)[NSUM], int n, double eps) {
    const double dn = (double)n;
    double v;
    if (MODE == 0) {
        v = nef_wave_sum_d(s[0]) / dn;
    } else {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) s[k] = nef_wave_sum_d(s[k]);
        const double mu = s[0] / dn, mw = s[1] / dn;
        const double vx = s[2] / dn - mu * mu;
        const double vy = s[3] / dn - mw * mw;
        const double c = s[4] / dn - mu * mw;
        v = 1.0 - (c + eps) / sqrt((vx + eps) * (vy + eps));
    }
    return v != v ? (double)INFINITY : v;
}

// grid B * tilesA blocks of 256 threads: wave w of block (b, tile) owns candidate tile * 4 + w of sample b
template <int MODE>
__global__ __launch_bounds__(256) void locate_score_kernel(const nef_locate_score_args a, int tilesA) {
    const int lane = threadIdx.x & 63;
    const int b = (int)(blockIdx.x / (unsigned)tilesA);
    const int cand = ((int)blockIdx.x - b * tilesA) * 4 + (int)(threadIdx.x >> 6);
    if (cand >= a.A) return;                              // wave-uniform; the block has no barrier
    const int n = nef_row_end(a.rois, b, a.L);
    const int G = a.group;
    const int r_lo = G ? cand / G : 0, r_hi = G ? r_lo + 1 : a.R;
    double* out = a.scores + (int64_t)b * a.sc_bs + a.col_off + (G ? cand - r_lo * G : cand);
    if (n < (MODE == 0 ? 1 : 2)) {                        // a row that does not count
        if (lane == 0)
            for (int r = r_lo; r < r_hi; ++r) out[(int64_t)r * a.sc_rs] = (double)INFINITY;
        return;
    }
    const float* p = a.pred + (int64_t)b * a.pred_bs + (int64_t)cand * a.pred_as;
    const bool pvec = ((uintptr_t)p & 15) == 0;
    const double p0 = (double)p[0];
    const bool one = n <= SEG;                            // the whole row in registers: read once for all R observed rows
    Seg ps;
    if (one) ps = load_seg(p, 0, n, lane, pvec);
    for (int r = r_lo; r < r_hi; ++r) {
        const float* y = a.obs + (int64_t)b * a.obs_bs + (int64_t)r * a.obs_rs;
        const bool yvec = ((uintptr_t)y & 15) == 0;
        const double y0 = (double)y[0];
        double s[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < n; k0 += SEG) {
            if (!one) ps = load_seg(p, k0, n, lane, pvec);
            const Seg ys = load_seg(y, k0, n, lane, yvec);
            add_seg<MODE>(s, ps, ys, k0, n, lane, p0, y0);
        }
        const double v = finish<MODE>(s, n, a.eps);
        if (lane == 0) out[(int64_t)r * a.sc_rs] = v;
    }
}

// one wave per (sample, observed row): lane l scans columns l, l + 64, ... in rising order, then a butterfly on (score, column) in
// lexicographic order -- the earliest column among equal scores, whatever the lane it sat in
__global__ __launch_bounds__(256) void locate_best_kernel(const nef_locate_best_args a) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (int64_t)a.B * a.R) return;               // wave-uniform
    const int b = (int)(pair / a.R), r = (int)(pair - (int64_t)b * a.R);
    const double* sc = a.scores + (int64_t)b * a.sc_bs + (int64_t)r * a.sc_rs;
    const double inf = (double)INFINITY;
    double bs = inf;
    int bj = -1;                                          // -1 <=> bs == inf: only a finite score is strictly lower than +inf
    for (int j = lane; j < a.A; j += NEF_WAVE) {
        double v = sc[j];
        if (v != v) v = inf;
        if (v < bs) bs = v, bj = j;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(bs, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (os < bs || (os == bs && oj >= 0 && oj < bj)) bs = os, bj = oj;
    }
    if (lane != 0) return;
    double cur = inf;
    if (!a.init) {
        if (a.keep_index && a.best_index[pair] < 0) return;      // no finite level-0 score: stays as it is
        cur = a.best_score[pair];
        if (cur != cur) cur = inf;
    }
    if (bj >= 0 && bs < cur) {
        const float* c = a.cands + ((a.per_pair ? pair * a.A : (int64_t)0) + bj) * 2;
        a.best_score[pair] = bs;
        a.best_theta[pair * 2 + 0] = c[0];
        a.best_theta[pair * 2 + 1] = c[1];
        if (!a.keep_index) a.best_index[pair] = a.index_base + bj;
    } else if (a.init) {
        a.best_score[pair] = inf;
        a.best_theta[pair * 2 + 0] = NAN;
        a.best_theta[pair * 2 + 1] = NAN;
        a.best_index[pair] = -1;
    }
}

// one thread per candidate
__global__ __launch_bounds__(256) void locate_cands_kernel(const nef_locate_cands_args a, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int W = 2 * a.radius + 1, G = W * W;
    const int64_t pair = idx / G;
    const int g = (int)(idx - pair * G);
    const int i = g / W, k = g - i * W;
    const bool found = a.best_index[pair] >= 0;
    const float c1 = found ? a.best_theta[pair * 2 + 0] : a.ph1;
    const float c2 = found ? a.best_theta[pair * 2 + 1] : a.ph2;
    a.cands[idx * 2 + 0] = __fadd_rn(c1, __fmul_rn((float)(i - a.radius), a.s1));
    a.cands[idx * 2 + 1] = __fadd_rn(c2, __fmul_rn((float)(k - a.radius), a.s2));
}

}  // namespace

extern "C" {

size_t nef_locate_score_args_bytes(void) { return sizeof(nef_locate_score_args); }
size_t nef_locate_best_args_bytes(void) { return sizeof(nef_locate_best_args); }
size_t nef_locate_cands_args_bytes(void) { return sizeof(nef_locate_cands_args); }

int nef_locate_score(const nef_locate_score_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->pred && a->obs && a->scores, NEF_E_NULL);
    NEF_REQUIRE(a->B >= 1 && a->A >= 1 && a->R >= 1 && a->L >= 1 && a->L <= (1 << 30), NEF_E_SHAPE);
    NEF_REQUIRE(a->group >= 0 && (a->group == 0 || (int64_t)a->R * a->group == a->A), NEF_E_SHAPE);
    NEF_REQUIRE(a->mode == 0 || a->mode == 1, NEF_E_SHAPE);
    NEF_REQUIRE(a->eps > 0.0 && a->eps < (double)INFINITY, NEF_E_SHAPE);              // (NaN fails >)
    NEF_REQUIRE(a->pred_bs >= 0 && a->pred_as >= 0 && a->obs_bs >= 0 && a->obs_rs >= 0 && a->sc_bs >= 0 && a->sc_rs >= 0 && a->col_off >= 0,
                NEF_E_SHAPE);
    const int64_t tilesA = nef_cdiv(a->A, 4);
    NEF_REQUIRE((int64_t)a->B * tilesA <= 0x7FFFFFFFll, NEF_E_SHAPE);
    const dim3 grid((unsigned)((int64_t)a->B * tilesA));
    if (a->mode == 0)
        hipLaunchKernelGGL(locate_score_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, *a, (int)tilesA);
    else
        hipLaunchKernelGGL(locate_score_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, *a, (int)tilesA);
    return nef_launch_status();
}

int nef_locate_best(const nef_locate_best_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->scores && a->cands && a->best_score && a->best_theta && a->best_index, NEF_E_NULL);
    NEF_REQUIRE(a->B >= 1 && a->R >= 1 && a->A >= 1 && (int64_t)a->B * a->R <= 0x7FFFFFFFll, NEF_E_SHAPE);
    NEF_REQUIRE(a->sc_bs >= 0 && a->sc_rs >= 0 && a->index_base >= 0, NEF_E_SHAPE);
    const int64_t pairs = (int64_t)a->B * a->R;
    hipLaunchKernelGGL(locate_best_kernel, dim3((unsigned)nef_cdiv(pairs, 4)), dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

int nef_locate_cands(const nef_locate_cands_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->best_theta && a->best_index && a->cands, NEF_E_NULL);
    NEF_REQUIRE(a->B >= 1 && a->R >= 1 && a->radius >= 0 && a->radius <= 16, NEF_E_SHAPE);
    const float lim = INFINITY;
    NEF_REQUIRE(fabsf(a->s1) < lim && fabsf(a->s2) < lim && fabsf(a->ph1) < lim && fabsf(a->ph2) < lim, NEF_E_SHAPE);   // (NaN fails <)
    const int W = 2 * a->radius + 1;
    const int64_t total = (int64_t)a->B * a->R * W * W;
    NEF_REQUIRE(total <= 0x7FFFFFFFll, NEF_E_SHAPE);
    hipLaunchKernelGGL(locate_cands_kernel, dim3((unsigned)nef_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, *a, total);
    return nef_launch_status();
}

}  // extern "C"
