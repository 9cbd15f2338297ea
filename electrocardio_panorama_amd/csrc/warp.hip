// Time warp of a train batch with jittered marks (cfg.DATA.aug_warp / aug_roi_jitter): every segment of every beat resampled to a drawn
// multiple of its length -- input leads, target and rest views alike -- and the marks moved with it.  Definition, step by step:
// include/nefnet_hip.h (nef_warp_args).  Every draw is a function of (seed, index0 + sample, segment) through nef_rng_mix: no state, no
// atomics, one writer per element.
//
// One 256-thread workgroup per sample.  The edge / length tables (7 + 7 + 6 words and 6 ratios) are formed by every thread from the
// sample's seven clamped marks and six draws: block-uniform, so they live in scalar registers.  A wave owns one row at a time, a lane four
// neighbouring output positions: the segment of a position comes from a select chain over the new edges (no indexed private array, no
// scratch), its two source samples from two 4-byte gathers out of a row that is in L1 / L2 after the first touch, the blend is fp64,
// the store 16 bytes.
#include "nef_common.h"

namespace {

constexpr double INV24 = 1.0 / 16777216.0;
constexpr uint64_t SAMPLE_BASE = 1ull << 62;

__device__ __forceinline__ int clampi(int64_t v, int64_t lo, int64_t hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

__global__ __launch_bounds__(256) void warp_kernel(const nef_warp_args a) {
    const int b = (int)blockIdx.x, L = a.L;
    const int64_t* __restrict__ roi = a.rois + (int64_t)b * 14;

    // 1. sanitised edges: only these clamped values enter any arithmetic or address
    int c[7];
    c[0] = clampi(roi[0], 0, L);
#pragma unroll
    for (int k = 1; k < 7; ++k) {
        const int64_t s = roi[2 * k];
        c[k] = clampi(s > c[k - 1] ? s : (int64_t)c[k - 1], 0, L);
    }
    const bool cropped = c[6] == L;

    // 2. - 4. draws, new lengths, new edges; 6. marks
    const uint64_t ctr = SAMPLE_BASE + 8ull * (uint64_t)(a.index0 + (int64_t)b);
    int n[6], d[7], e[7];
    double r[6];
    d[0] = c[0];
    e[0] = c[0];
    int jit[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint64_t z = nef_rng_mix(a.seed, ctr + (uint64_t)k);
        const double u = (double)(uint32_t)(z >> 40) * INV24;
        const double s = 1.0 + a.amp[k] * (2.0 * u - 1.0);
        n[k] = c[k + 1] - c[k];
        int64_t m = 0;
        if (n[k] > 0) {
            m = cropped ? (int64_t)n[k] : (int64_t)floor((double)n[k] * s + 0.5);
            if (m < 1) m = 1;
        }
        r[k] = m > 0 ? (double)n[k] / (double)m : 0.0;
        const int64_t nd = (int64_t)d[k] + m;
        d[k + 1] = (int)(nd < L ? nd : (int64_t)L);
        jit[k] = (int)(((uint64_t)(2 * a.jitter + 1) * ((z >> 16) & 0xFFFFFFull)) >> 24) - a.jitter;
    }
#pragma unroll
    for (int k = 1; k < 6; ++k) e[k] = clampi((int64_t)d[k] + jit[k], e[k - 1], d[6]);
    e[6] = d[6];

    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    if (wave == 0 && lane < 14) {                      // rois_out[b, k] = [e_k, e_{k+1}]; the last end passes through as given
        int64_t v = roi[13];
#pragma unroll
        for (int q = 0; q < 13; ++q)
            if (lane == q) v = e[(q + 1) >> 1];
        a.rois_out[(int64_t)b * 14 + lane] = v;
    }

    // 5. values: rows 0 .. V - 1 the inputs, V the target, V + 1 .. V + R the rest views
    const int rows = a.V + 1 + a.R;
    for (int row = wave; row < rows; row += 4) {
        const float* __restrict__ x;
        float* __restrict__ y;
        if (row < a.V) {
            const int64_t o = ((int64_t)b * a.V + row) * L;
            x = a.data + o;
            y = a.data_out + o;
        } else if (row == a.V) {
            x = a.target + (int64_t)b * L;
            y = a.target_out + (int64_t)b * L;
        } else {
            const int64_t o = ((int64_t)b * a.R + (row - a.V - 1)) * L;
            x = a.rest + o;
            y = a.rest_out + o;
        }
        for (int t0 = lane * 4; t0 < L; t0 += 256) {    // L % 4 == 0: the four positions are inside the row
            float out[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int t = t0 + q;
                float v = 0.f;
                if (t < d[0]) {
                    v = x[t];
                } else if (t < d[6]) {
                    int ck = c[0], dk = d[0], nk = n[0];
                    double rk = r[0];
#pragma unroll
                    for (int k = 1; k < 6; ++k)
                        if (t >= d[k]) {
                            ck = c[k];
                            dk = d[k];
                            nk = n[k];
                            rk = r[k];
                        }
                    // d_k <= t < d_{k+1} implies m_k > 0, hence n_k >= 1 and c_k + n_k <= L
                    double p = ((double)(t - dk) + 0.5) * rk - 0.5;
                    const double hi = (double)(nk - 1);
                    p = p < 0.0 ? 0.0 : (p > hi ? hi : p);
                    const double fl = floor(p);
                    const int i0 = (int)fl;
                    const int i1 = i0 + 1 < nk ? i0 + 1 : nk - 1;
                    const double f = p - fl;
                    const double x0 = (double)x[ck + i0], x1 = (double)x[ck + i1];
                    v = f == 0.0 ? (float)x0 : (float)(x0 + f * (x1 - x0));
                }
                out[q] = v;
            }
            *reinterpret_cast<float4*>(y + t0) = make_float4(out[0], out[1], out[2], out[3]);
        }
    }
}

// [p, p + bytes) and [q, q + qbytes) share a byte
inline bool overlaps(const void* p, uintptr_t bytes, const void* q, uintptr_t qbytes) {
    const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
    return p && q && p0 < q0 + qbytes && q0 < p0 + bytes;
}

}  // namespace

extern "C" {

size_t nef_warp_args_bytes(void) { return sizeof(nef_warp_args); }

int nef_warp(const nef_warp_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->data && a->target && a->rois && a->data_out && a->target_out && a->rois_out, NEF_E_NULL);
    NEF_REQUIRE(a->R == 0 || (a->rest && a->rest_out), NEF_E_NULL);
    NEF_REQUIRE(a->B >= 1 && a->V >= 1 && a->V <= 12 && a->R >= 0 && a->R <= 64, NEF_E_SHAPE);
    NEF_REQUIRE(a->L >= 4 && a->L <= (1 << 24) && a->L % 4 == 0, NEF_E_SHAPE);
    NEF_REQUIRE(a->jitter >= 0 && a->jitter <= NEF_WARP_MAX_JITTER, NEF_E_SHAPE);
    for (int k = 0; k < 6; ++k) NEF_REQUIRE(a->amp[k] >= 0.0 && a->amp[k] <= NEF_WARP_MAX_AMP, NEF_E_SHAPE);      // (NaN fails both)
    const void* in[4] = {a->data, a->target, a->R ? a->rest : nullptr, a->rois};
    const void* out[4] = {a->data_out, a->target_out, a->R ? a->rest_out : nullptr, a->rois_out};
    const uintptr_t row = (uintptr_t)a->L * sizeof(float), B = (uintptr_t)a->B;
    const uintptr_t bytes[4] = {B * (uintptr_t)a->V * row, B * row, B * (uintptr_t)a->R * row, B * 14 * sizeof(int64_t)};
    uintptr_t bits = 0;
    for (int i = 0; i < 4; ++i) bits |= (uintptr_t)in[i] | (uintptr_t)out[i];
    NEF_REQUIRE((bits & 15) == 0, NEF_E_UNSUPPORTED);
    for (int o = 0; o < 4; ++o) {
        for (int i = 0; i < 4; ++i) NEF_REQUIRE(!overlaps(out[o], bytes[o], in[i], bytes[i]), NEF_E_UNSUPPORTED);
        for (int i = 0; i < o; ++i) NEF_REQUIRE(!overlaps(out[o], bytes[o], out[i], bytes[i]), NEF_E_UNSUPPORTED);   // one writer per element
    }
    hipLaunchKernelGGL(warp_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

}  // extern "C"
