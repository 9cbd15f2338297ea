// The train step's label-noise row, made on the device (cfg.DATA.device_noise): out [Rw, L] = sigma_row * z, sigma_row the standard
// deviation of the quiet second half of the row's T-P segment, taken from the TARGET row itself, z the Box-Muller pair stream of
// nef_augment under this launch's seed.  Definition: include/nefnet_hip.h (nef_noise_row_args).  No state, no atomics, no scratch, one
// writer per element: the eager step, the replayed step (seed_dev) and a resumed run see the same bits.
//
// One 256-thread workgroup per row.  Phase 1 reduces the quiet segment twice in fp64 (mean, then the squared deviations): a thread sums
// its own elements in ascending order -- 16-byte loads over the aligned body of the segment, 4-byte loads at its two edges --, then the
// shuffle tree of nef_wave_sum_d, then the four waves in order through LDS (nef_block_sum_d): the order is a function of the segment
// alone.  Phase 2 writes the row: a thread owns four neighbouring positions per trip = two noise words and one 16-byte store.
#include "nef_common.h"
#include "aug_drop.h"

namespace {

using namespace nef_aug;      // field0 / field1 / INV24F: the noise words are cut as nef_augment cuts them

// sum over [a, b) of f(row[t]) in fp64, all threads get it.  a <= b, both inside the row; the row base is 16-byte aligned.
template <class F>
__device__ __forceinline__ double segment_sum(const float* __restrict__ row, int a, int b, double* sm, F f) {
    const int a4 = min((a + 3) & ~3, b);          // [a, a4): the unaligned head (up to three elements, or the whole short segment)
    const int b4 = max(b & ~3, a4);               // [a4, b4): whole 16-byte groups; [b4, b): the tail (up to three elements)
    const int tid = (int)threadIdx.x;
    double s = 0.0;
    if (a + tid < a4) s += f(row[a + tid]);
    for (int t = a4 + 4 * tid; t < b4; t += 4 * 256) {
        const float4 v = *reinterpret_cast<const float4*>(row + t);
        s += f(v.x);
        s += f(v.y);
        s += f(v.z);
        s += f(v.w);
    }
    if (b4 + tid < b) s += f(row[b4 + tid]);
    return nef_block_sum_d(s, sm);
}

__global__ __launch_bounds__(256) void noise_row_kernel(const nef_noise_row_args a) {
    __shared__ double sm[8];
    const int row = (int)blockIdx.x, L = a.L;
    const float* __restrict__ x = a.target + (int64_t)row * L;
    const int64_t* __restrict__ r = a.rois + (int64_t)row * 14;
    const int end = nef_row_end(a.rois, row, L);                    // clamp(rois[row, -1, 0], 0, L)
    // the quiet segment: [floor((s + e) / 2), e) of rois[row, 5] = (s, e), cut to [0, end).  The halves are added, not the sum halved:
    // no int64 content overflows, and >> is the true floor of a negative value.  Only the clamped ends reach an address
    const int64_t s5 = r[10], e5 = r[11];
    const int64_t mid = (s5 >> 1) + (e5 >> 1) + (((s5 & 1) + (e5 & 1)) >> 1);
    const int q0 = mid < 0 ? 0 : (mid > end ? end : (int)mid);
    const int q1 = e5 < 0 ? 0 : (e5 > end ? end : (int)e5);
    const int m = q1 > q0 ? q1 - q0 : 0;

    double sigma = 0.0;
    if (m > 0) {                                                    // (block-uniform)
        const double mean = segment_sum(x, q0, q1, sm, [](float v) { return (double)v; }) / (double)m;
        const double ss = segment_sum(x, q0, q1, sm + 4, [mean](float v) { const double d = (double)v - mean; return d * d; });
        sigma = sqrt(ss / (double)m);
    }
    if (a.sigma && threadIdx.x == 0) a.sigma[row] = sigma;

    const float sf = (float)sigma;
    const bool zero = sf == 0.f;                                    // (false for a NaN: the row is NaN up to its end)
    const uint64_t seed = a.seed + (a.seed_dev ? a.seed_dev[0] : 0ull);
    const int64_t e0 = (int64_t)row * L;                            // dense element index of the row's first position, a multiple of 4
    float4* __restrict__ out = reinterpret_cast<float4*>(a.out + e0);
    for (int t0 = 4 * (int)threadIdx.x; t0 < L; t0 += 4 * 256) {
        float y[4] = {0.f, 0.f, 0.f, 0.f};
        if (!zero && t0 < end) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const uint64_t z = nef_rng_mix(seed, (uint64_t)((e0 + t0) >> 1) + p);
                const float rr = sqrtf(-2.0f * logf((float)(field0(z) + 1u) * INV24F));
                float s, c;
                sincospif(2.0f * ((float)field1(z) * INV24F), &s, &c);
                y[2 * p] = sf * (rr * c);
                y[2 * p + 1] = sf * (rr * s);
            }
        }
        // a row end inside these four positions (it may split a noise pair): the positions at or behind it are +0.0
        out[t0 >> 2] = make_float4(t0 < end ? y[0] : 0.f, t0 + 1 < end ? y[1] : 0.f, t0 + 2 < end ? y[2] : 0.f, t0 + 3 < end ? y[3] : 0.f);
    }
}

}  // namespace

extern "C" {

size_t nef_noise_row_args_bytes(void) { return sizeof(nef_noise_row_args); }

int nef_noise_row(const nef_noise_row_args* a, nef_stream_t stream) {
    NEF_ENTER();
    NEF_REQUIRE(a && a->target && a->rois && a->out, NEF_E_NULL);
    NEF_REQUIRE(a->Rw >= 1 && a->L > 0 && a->L % 4 == 0, NEF_E_SHAPE);
    const uintptr_t x0 = (uintptr_t)a->target, y0 = (uintptr_t)a->out, bytes = (uintptr_t)a->Rw * (uintptr_t)a->L * sizeof(float);
    NEF_REQUIRE(((x0 | y0) & 15) == 0 && ((uintptr_t)a->rois & 7) == 0 && ((uintptr_t)a->sigma & 7) == 0 && ((uintptr_t)a->seed_dev & 7) == 0,
                NEF_E_UNSUPPORTED);
    NEF_REQUIRE(x0 + bytes <= y0 || y0 + bytes <= x0, NEF_E_UNSUPPORTED);
    hipLaunchKernelGGL(noise_row_kernel, dim3((unsigned)a->Rw), dim3(256), 0, (hipStream_t)stream, *a);
    return nef_launch_status();
}

}  // extern "C"
